// The header formatter, the batch planner and the splice of the chain files (sweepga_amd/csrc/host/ucsc_text.cpp) without a GPU and
// without the library: a stand-alone program meant to be built with the host sanitizers, together with ucsc_text.cpp and
// cigar_text.cpp.  Standard input, case by case:
//   H <newline> nine numbers: score flags ref_start ref_end oth_start oth_end ref_size oth_size id <newline> reference name <newline>
//     other name                        ->  the header line
//   P <newline> batch_bytes k len_0 .. len_{k-1}   ->  the batches' first entries and k, space-separated, one line
//   S <newline> k text_bytes, then per row `n_blocks text_first header-without-its-newline`, then the text with '|' for '\n', each
//     on a line                         ->  the spliced bytes with '|' for '\n', one line.  The rows, the headers and the text are
//     copied into heap blocks of exactly their size first, so that a read past either end is the address sanitizer's to find.
// tests/test_ucsc_chain_cpu.py feeds it and compares the bytes with tests/ucsc_chain_model.py.
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

// what the PAF seams of ucsc_text.cpp link against; nothing here calls them
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
int swg_ucsc_run(swg_ctx*, const swg_records*, bool, const uint32_t*, const uint8_t*, const swg_cigar_set*, swg_ucsc_request*) { std::abort(); }
uint64_t swg_ucsc_default_batch(swg_ctx*) { std::abort(); }

int main() {
  std::string kind, line;
  while (std::getline(std::cin, kind)) {
    if (kind == "H") {
      std::string ref, oth;
      if (!std::getline(std::cin, line) || !std::getline(std::cin, ref) || !std::getline(std::cin, oth)) return 2;
      std::istringstream in(line);
      uint64_t v[9];
      for (uint64_t& x : v)
        if (!(in >> x)) return 2;
      swg_ucsc_chain ch{};
      ch.score = (uint32_t)v[0], ch.flags = (uint32_t)v[1], ch.ref_start = (uint32_t)v[2], ch.ref_end = (uint32_t)v[3];
      ch.oth_start = (uint32_t)v[4], ch.oth_end = (uint32_t)v[5];
      std::string o;
      swg_ucsc_header_text(o, ch, ref.c_str(), v[6], oth.c_str(), v[7], v[8]);
      std::fwrite(o.data(), 1, o.size(), stdout);
    } else if (kind == "P") {
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream in(line);
      uint64_t batch, k;
      if (!(in >> batch >> k)) return 2;
      uint64_t* len = static_cast<uint64_t*>(std::malloc(k ? k * sizeof(uint64_t) : 1));
      if (!len) return 3;
      for (uint64_t j = 0; j < k; ++j)
        if (!(in >> len[j])) return 2;
      std::vector<uint64_t> first;
      swg_ucsc_plan_batches(len, k, batch, &first);
      std::free(len);
      for (size_t b = 0; b < first.size(); ++b) std::printf(b ? " %llu" : "%llu", (unsigned long long)first[b]);
      std::fputc('\n', stdout);
    } else if (kind == "S") {
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream in(line);
      uint64_t k, text_bytes;
      if (!(in >> k >> text_bytes)) return 2;
      swg_ucsc_chain* rows = static_cast<swg_ucsc_chain*>(std::malloc(k ? k * sizeof(swg_ucsc_chain) : 1));
      if (!rows) return 3;
      std::vector<std::string> hdr(k);
      for (uint64_t j = 0; j < k; ++j) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream row(line);
        unsigned long long nb, tf;
        if (!(row >> nb >> tf)) return 2;
        std::memset(&rows[j], 0, sizeof rows[j]);
        rows[j].n_blocks = (uint32_t)nb, rows[j].text_first = tf;
        std::getline(row, hdr[j]);
        if (!hdr[j].empty()) hdr[j] = hdr[j].substr(1) + "\n";
      }
      if (!std::getline(std::cin, line) || line.size() != text_bytes) return 2;
      char* text = static_cast<char*>(std::malloc(text_bytes ? text_bytes : 1));
      if (!text) return 3;
      for (uint64_t b = 0; b < text_bytes; ++b) text[b] = line[b] == '|' ? '\n' : line[b];
      std::string out;
      swg_ucsc_sink sink;
      sink.text = &out;
      swg_ucsc_splice(&sink, rows, k, hdr.data(), text, text_bytes);
      std::free(text);
      std::free(rows);
      for (char& ch : out)
        if (ch == '\n') ch = '|';
      std::fwrite(out.data(), 1, out.size(), stdout);
      std::fputc('\n', stdout);
    } else {
      return 2;
    }
  }
  return 0;
}
