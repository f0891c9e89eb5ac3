// The formatters and the batch merge of the divergence track (sweepga_amd/csrc/host/divergence_text.cpp) without a GPU and without
// the library: a stand-alone program meant to be built with the host sanitizers, together with divergence_text.cpp, ucsc_text.cpp and
// cigar_text.cpp.  Standard input, case by case:
//   R <newline> name <newline> twelve numbers: seq start end n and the eight sums   ->  the rows header and the row's line
//   S <newline> name <newline> length, then twelve numbers: seq windows records entries and the eight sums
//                                                                                  ->  the summary header and the sequence's line
//   M <newline> b <newline> per batch: n <newline> n lines of twelve numbers        ->  the b batches merged as rows: one line of twelve
//                                                                                      numbers per row, or `refused`; then `--`
//   Q <newline> b <newline> per batch: n <newline> n lines of twelve numbers        ->  the same for summary entries
// Every batch is a vector of exactly its size, so that a read past its end is the address sanitizer's to find.
// tests/test_divergence_cpu.py feeds it and compares the bytes with tests/divergence_model.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

// what the PAF seams of divergence_text.cpp and ucsc_text.cpp link against; nothing here calls them
int swg_alnstats_error(int code, const char*, ...) { return code; }
extern "C" {
const char* swg_last_error(const swg_ctx*) { std::abort(); }
const swg_records* swg_paf_records(const swg_paf*) { std::abort(); }
const uint64_t* swg_paf_seq_offsets(const swg_paf*) { std::abort(); }
const uint64_t* swg_paf_record_offsets(const swg_paf*, int) { std::abort(); }
const char* swg_paf_sequence_name(const swg_paf*, uint32_t) { std::abort(); }
}
int swg_paf_seq_last_lengths(const swg_paf*, std::vector<uint32_t>*) { std::abort(); }
void swg_paf_lines_view(const swg_paf*, const char**, const uint64_t**, const uint32_t**) { std::abort(); }
void swg_paf_stats_genome_names(const swg_paf*, std::vector<std::string>*) { std::abort(); }
int swg_ucsc_run(swg_ctx*, const swg_records*, bool, const uint32_t*, const uint8_t*, const swg_cigar_set*, swg_ucsc_request*) { std::abort(); }
int swg_divergence_run(swg_ctx*, const swg_records*, bool, const uint32_t*, const uint32_t*, uint32_t, const uint8_t*, const swg_cigar_set*,
                       swg_divergence_request*, std::vector<swg_divergence_row>*, std::vector<swg_divergence_seq>*) {
  std::abort();
}
uint64_t swg_ucsc_default_batch(swg_ctx*) { std::abort(); }

static bool numbers(uint64_t* v, int count) {
  std::string line;
  if (!std::getline(std::cin, line)) return false;
  std::istringstream in(line);
  for (int f = 0; f < count; ++f) {
    unsigned long long x;
    if (!(in >> x)) return false;
    v[f] = x;
  }
  return true;
}

static swg_divergence_row row_of(const uint64_t* v) {
  return swg_divergence_row{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
}
static swg_divergence_seq seq_of(const uint64_t* v) {
  return swg_divergence_seq{(uint32_t)v[0], (uint32_t)v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
}

template <class Row, class Make, class Merge, class Print>
static int merge_case(Make make, Merge merge, Print print) {
  uint64_t b, n, v[12];
  if (!numbers(&b, 1)) return 2;
  std::vector<Row> total;
  bool fine = true;
  for (uint64_t k = 0; k < b; ++k) {
    if (!numbers(&n, 1)) return 2;
    std::vector<Row> add;
    add.reserve(n);
    for (uint64_t j = 0; j < n; ++j) {
      if (!numbers(v, 12)) return 2;
      add.push_back(make(v));
    }
    const std::vector<Row> exact(add.begin(), add.end());  // (capacity = size)
    if (fine) fine = merge(&total, exact, k == 0);
  }
  if (!fine) std::puts("refused");
  else
    for (const Row& r : total) print(r);
  std::puts("--");
  return 0;
}

int main() {
  std::string kind, name;
  uint64_t v[13];
  while (std::getline(std::cin, kind)) {
    if (kind == "R") {
      if (!std::getline(std::cin, name) || !numbers(v, 12)) return 2;
      std::string o;
      swg_divergence_rows_header(o);
      swg_divergence_row_text(o, name.c_str(), row_of(v));
      std::fwrite(o.data(), 1, o.size(), stdout);
    } else if (kind == "S") {
      if (!std::getline(std::cin, name) || !numbers(v, 13)) return 2;
      std::string o;
      swg_divergence_summary_header(o);
      swg_divergence_seq_text(o, name.c_str(), v[0], seq_of(v + 1));
      std::fwrite(o.data(), 1, o.size(), stdout);
    } else if (kind == "M") {
      const int rc = merge_case<swg_divergence_row>(row_of, swg_divergence_merge_rows, [](const swg_divergence_row& r) {
        std::printf("%u %u %u %u", r.seq, r.start, r.end, r.n);
        const uint64_t* s = &r.aligned;
        for (int f = 0; f < 8; ++f) std::printf(" %llu", (unsigned long long)s[f]);
        std::fputc('\n', stdout);
      });
      if (rc) return rc;
    } else if (kind == "Q") {
      const int rc = merge_case<swg_divergence_seq>(seq_of, swg_divergence_merge_seqs, [](const swg_divergence_seq& r) {
        std::printf("%u %u", r.seq, r.windows);
        const uint64_t* s = &r.records;
        for (int f = 0; f < 10; ++f) std::printf(" %llu", (unsigned long long)s[f]);
        std::fputc('\n', stdout);
      });
      if (rc) return rc;
    } else {
      return 2;
    }
  }
  return 0;
}
