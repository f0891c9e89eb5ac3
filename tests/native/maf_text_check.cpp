// The block formatter of sweepga_amd/csrc/host/maf_text.cpp on its own: a stand-alone program that a host compiler builds from that
// file (with ucsc_text.cpp and cigar_text.cpp for the sink, the planner and the tag search; it needs neither the library nor a device:
// the few symbols of the library that the entry points it never calls name are defined below).  Standard input: blocks of three lines
// -- a PAF line, `t_start t_bases q_start q_bases aligned columns flags`, the two rows end to end (`.` = none); for each it prints
// the MAF block under the line's own names.  A first argument `long` adds a block whose names have 100,000 bytes each and whose rows
// have 70,000 columns.  tests/test_maf_cpu.py builds it with -fsanitize=address,undefined, runs it and compares every block with
// tests/maf_model.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

static std::string field(const std::string& line, int want) {
  size_t at = 0;
  for (int f = 0; f < want; ++f) at = line.find('\t', at) + 1;
  return line.substr(at, line.find('\t', at) - at);
}

static void one(const std::string& line, const swg_maf_block& b, const std::string& rows) {
  // exactly the line's and the rows' bytes on the heap: a read past either end is the sanitizer's
  std::vector<char> L(line.begin(), line.end()), R(rows.begin(), rows.end());
  std::string o;
  swg_maf_block_text(o, field(line, 5).c_str(), field(line, 0).c_str(), L.data(), L.size(), b, R.data());
  std::fwrite(o.data(), 1, o.size(), stdout);
}

int main(int argc, char** argv) {
  std::string line, numbers, rows;
  while (std::getline(std::cin, line) && std::getline(std::cin, numbers) && std::getline(std::cin, rows)) {
    swg_maf_block b{};
    if (std::sscanf(numbers.c_str(), "%u %u %u %u %u %u %u", &b.t_start, &b.t_bases, &b.q_start, &b.q_bases, &b.aligned, &b.columns, &b.flags) != 7) return 2;
    if (rows == ".") rows.clear();
    if (rows.size() != 2 * (size_t)b.columns) return 3;
    one(line, b, rows);
  }
  if (argc > 1 && std::string(argv[1]) == "long") {
    const std::string q(100000, 'q'), t(100000, 't');
    swg_maf_block b{};
    b.t_start = 4294900000u, b.t_bases = 67295u, b.q_start = 5u, b.q_bases = 70000u, b.aligned = 67295u, b.columns = 70000u, b.flags = SWG_MAF_MINUS;
    one(q + "\t4294967295\t5\t70005\t-\t" + t + "\t4294967295\t4294900000\t4294967295\t1\t2\t60\tcg:Z:1M", b, std::string(70000, 'A') + std::string(70000, 'c'));
  }
  return 0;
}

// ---- what maf_text.cpp's entry points name and this program never reaches -------------------------------------------------------------
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
int swg_maf_run(swg_ctx*, const swg_records*, int, const uint8_t*, const swg_cigar_set*, const swg_seq_set*, swg_maf_request*) { return 0; }
int swg_variant_bases_upload(swg_ctx*, const uint8_t* const*, const uint64_t*, uint32_t, uint64_t*, uint8_t**) { return 0; }
void swg_variant_bases_free(swg_ctx*, uint8_t*) {}
