// The line formatter of sweepga_amd/csrc/host/eqx_text.cpp on its own: a stand-alone program that a host compiler builds from that
// file (with ucsc_text.cpp and cigar_text.cpp for the sink and the tag search; it needs neither the library nor a device: the few symbols
// of the library that the entry points it never calls name are defined below).  Standard input: blocks of three lines -- a PAF line,
// `matches block`, the new text (`-` = empty); for each it finds the line's last cg:Z: tag as the seam does and prints the rewritten
// line.  A first argument `long` adds a line whose names have 100,000 bytes each.  tests/test_eqx_cpu.py builds it with
// -fsanitize=address,undefined, runs it and compares every line with tests/eqx_model.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

static void one(const std::string& line, uint64_t matches, uint64_t block, const std::string& text) {
  // exactly the line's bytes on the heap: a read past either end is the sanitizer's
  std::vector<char> L(line.begin(), line.end()), T(text.begin(), text.end());
  uint64_t cg_len = 0;
  const char* cg = swg_cigar_tag_find(L.data(), L.size(), &cg_len);
  if (!cg) {
    std::puts("NO-TAG");
    return;
  }
  std::string o;
  swg_eqx_line_text(o, L.data(), L.size(), cg, cg_len, matches, block, T.data(), T.size());
  std::fwrite(o.data(), 1, o.size(), stdout);
}

int main(int argc, char** argv) {
  std::string line, numbers, text;
  while (std::getline(std::cin, line) && std::getline(std::cin, numbers) && std::getline(std::cin, text)) {
    unsigned long long matches = 0, block = 0;
    if (std::sscanf(numbers.c_str(), "%llu %llu", &matches, &block) != 2) return 2;
    one(line, matches, block, text == "-" ? std::string() : text);
  }
  if (argc > 1 && std::string(argv[1]) == "long") {
    const std::string q(100000, 'q'), t(100000, 't');
    one(q + "\t9\t0\t9\t-\t" + t + "\t9\t0\t9\t1\t2\t60\tNM:i:3\tcg:Z:9M\tzz:Z:" + q, 4294967295ull, 12884901885ull, std::string(70000, '=') + "1X");
  }
  return 0;
}

// ---- what eqx_text.cpp's entry points name and this program never reaches -------------------------------------------------------------
int swg_alnstats_error(int code, const char*, ...) { return code; }
const swg_records* swg_paf_records(const swg_paf*) { return nullptr; }
const uint64_t* swg_paf_seq_offsets(const swg_paf*) { return nullptr; }
const uint64_t* swg_paf_record_offsets(const swg_paf*, int) { return nullptr; }
const char* swg_paf_sequence_name(const swg_paf*, uint32_t) { return ""; }
int swg_paf_seq_last_lengths(const swg_paf*, std::vector<uint32_t>*) { return 0; }
void swg_paf_lines_view(const swg_paf*, const char**, const uint64_t**, const uint32_t**) {}
uint64_t swg_ucsc_default_batch(swg_ctx*) { return 0; }
uint64_t swg_fasta_num_records(const swg_fasta*) { return 0; }
const char* swg_fasta_name(const swg_fasta*, uint64_t) { return ""; }
const uint64_t* swg_fasta_offsets(const swg_fasta*) { return nullptr; }
const uint8_t* swg_fasta_bases(const swg_fasta*) { return nullptr; }
const char* swg_last_error(const swg_ctx*) { return ""; }
int swg_ucsc_run(swg_ctx*, const swg_records*, bool, const uint32_t*, const uint8_t*, const swg_cigar_set*, swg_ucsc_request*) { return 0; }
int swg_eqx_run(swg_ctx*, const swg_records*, int, const uint8_t*, const swg_cigar_set*, const swg_seq_set*, swg_eqx_request*) { return 0; }
int swg_variant_bases_upload(swg_ctx*, const uint8_t* const*, const uint64_t*, uint32_t, uint64_t*, uint8_t**) { return 0; }
void swg_variant_bases_free(swg_ctx*, uint8_t*) {}
