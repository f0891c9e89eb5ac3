// The formatters and the batch merge of sweepga_amd/csrc/host/variants_text.cpp on their own: a stand-alone program that a host
// compiler builds from that file (with ucsc_text.cpp and cigar_text.cpp for the sink and the tag search; it needs neither the library nor a device: the
// few symbols of the library that the entry points it never calls name are defined below).  It prints, one block after another, each closed by a line
// `--`: the header without and with a sample; lines with 10-digit positions, an empty and a very long name, names that need
// escaping, an allele of 10^5 bytes; the summary of two batches merged in both orders.  tests/test_variants_cpu.py builds it with
// -fsanitize=address,undefined, runs it and compares every block with tests/variants_model.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

static void block(const std::string& s) {
  std::fwrite(s.data(), 1, s.size(), stdout);
  std::puts("--");
}

static swg_variant_pair pair_of(uint32_t q, uint32_t t, uint64_t seed) {
  swg_variant_pair p{};
  p.q_genome = q, p.t_genome = t;
  uint64_t* v = &p.entries;
  for (int f = 0; f < 24; ++f) v[f] = seed * (f + 1) + (f == 7 ? 0xffffffffull : 0);
  p.snvs = 0;
  for (int i = 0; i < 12; ++i) p.snvs += p.sub[i];
  return p;
}

int main() {
  std::string o;
  swg_vcf_header_text(o, {"chr1", "g2#1#t"}, {4294967295ull, 9000}, nullptr);
  block(o);
  o.clear();
  swg_vcf_header_text(o, {}, {}, "g1#1#");
  block(o);

  const std::string long_name(5000, 'n');
  std::vector<uint8_t> big(100002, 'A');
  big[0] = 'C', big[1] = 'C', big[100001] = 'T';
  o.clear();
  swg_variant v{};
  v.record = 4294967295u, v.kind_flags = SWG_VARIANT_SNP, v.pos = 4294967294u, v.ref_len = 1, v.alt_len = 1, v.q_pos = 4294967295u;
  swg_vcf_line_text(o, "chr1", "q", v, reinterpret_cast<const uint8_t*>("AC"), false);
  v.kind_flags = SWG_VARIANT_SNP | SWG_VARIANT_MINUS;
  swg_vcf_line_text(o, "", "", v, reinterpret_cast<const uint8_t*>("GT"), true);
  v.record = 0, v.pos = 0, v.q_pos = 0, v.kind_flags = SWG_VARIANT_INS, v.alt_len = 100001;
  swg_vcf_line_text(o, long_name.c_str(), long_name.c_str(), v, big.data(), false);
  v.kind_flags = SWG_VARIANT_DEL | SWG_VARIANT_MINUS, v.ref_len = 100001, v.alt_len = 1;
  swg_vcf_line_text(o, "t", "a;b=c,d%e f\tg\x01h", v, big.data(), true);
  block(o);

  const std::vector<std::string> gname = {"g0#1#", "g1#1#", "g2"};
  const std::vector<swg_variant_pair> a = {pair_of(0, 1, 3), pair_of(1, 0, 5), pair_of(2, 2, 7)};
  const std::vector<swg_variant_pair> b = {pair_of(0, 0, 11), pair_of(1, 0, 13), pair_of(2, 2, 17)};
  for (int order = 0; order < 2; ++order) {
    std::vector<swg_variant_pair> total;
    const std::vector<swg_variant_pair>& first = order ? b : a;
    const std::vector<swg_variant_pair>& second = order ? a : b;
    swg_variants_merge_pairs(&total, first.data(), first.size());
    swg_variants_merge_pairs(&total, second.data(), second.size());
    swg_variants_merge_pairs(&total, nullptr, 0);
    block(swg_variants_summary_text(gname, total));
  }
  return 0;
}

// ---- what variants_text.cpp's entry points name and this program never reaches ------------------------------------------------------
int swg_alnstats_error(int code, const char*, ...) { return code; }
const swg_records* swg_paf_records(const swg_paf*) { return nullptr; }
const uint64_t* swg_paf_seq_offsets(const swg_paf*) { return nullptr; }
const uint64_t* swg_paf_record_offsets(const swg_paf*, int) { return nullptr; }
uint32_t swg_paf_num_genomes_two(const swg_paf*) { return 0; }
const char* swg_paf_genome_two_prefix(const swg_paf*, uint32_t) { return ""; }
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
int swg_variant_run(swg_ctx*, const swg_records*, int, const uint32_t*, uint32_t, const uint8_t*, const swg_cigar_set*, const swg_seq_set*, swg_variant_request*,
                    uint8_t*) {
  return 0;
}
int swg_variant_bases_upload(swg_ctx*, const uint8_t* const*, const uint64_t*, uint32_t, uint64_t*, uint8_t**) { return 0; }
void swg_variant_bases_free(swg_ctx*, uint8_t*) {}
int swg_variant_order(swg_ctx*, const uint64_t*, uint64_t, int, uint32_t*) { return 0; }
