// Shared by the host translation units of libsweepga_gpu.so; not part of the C ABI.
#ifndef SWG_HOST_INTERNAL_H
#define SWG_HOST_INTERNAL_H
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// open_paf_input (src/paf.rs:10-30): the whole input as text -- mmap for plain files, parallel BGZF / serial gzip
// inflate for .gz/.bgz (or the gzip magic), "-" = stdin.  *handle owns the bytes until swg_host_text_release.
// Errors: negative code, text in swg_paf_last_error().
int swg_host_text_load(const char* path, int threads, const char** data, size_t* len, void** handle);
void swg_host_text_release(void* handle);

// ---- the report writers' text helpers ----
inline void append_u64(std::string& o, uint64_t v, char sep) {  // v in decimal, then sep; no allocation of its own
  char buf[24];
  int k = 24;
  do buf[--k] = (char)('0' + v % 10); while (v /= 10);
  o.append(buf + k, 24 - k);
  o += sep;
}
// a text as the C ABI hands it out: malloc'd, NUL-terminated; nullptr = out of host memory
inline char* text_copy(const std::string& o) {
  char* t = static_cast<char*>(std::malloc(o.size() + 1));
  if (!t) return nullptr;
  std::memcpy(t, o.data(), o.size());
  t[o.size()] = 0;
  return t;
}

struct swg_ctx;
struct swg_fasta;
int swg_set_error(swg_ctx* ctx, int code, const char* fmt, ...);

// ---- alnstats on the device (swg_alnstats.hip, alnstats.cpp, paf_io.cpp) ----
#ifdef SWEEPGA_GPU_H
#include <string>
#include <vector>
// one result set of the device statistics with library-owned storage (the C ABI copies it into the caller's arrays)
struct swg_alnstats_result {
  uint64_t total_mappings = 0, total_bases = 0, total_matches = 0, self_mappings = 0, inter_chromosomal = 0, inter_genome = 0,
           chr_pair_count = 0;
  std::vector<swg_alnstats_pair_counts> pairs;  // ascending first_record
  std::vector<uint64_t> seq_last;               // [n_seq], UINT64_MAX = absent
};
// columns of rec on the host (on_device = false: staged in the arena) or on the device, seq_genome / status likewise
int swg_alnstats_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome,
                     const uint8_t* status, swg_alnstats_result* all, swg_alnstats_result* kept);
// an ordinary swg_alnstats handle from one result set: genome g's name (trailing '#' kept) and size (sum of the last-seen
// lengths of its sequences in the set); calculate_coverage_stats (:42-73) in the order of the pairs
int swg_alnstats_from_counts(const swg_alnstats_result& r, const std::vector<std::string>& genome_name,
                             const std::vector<uint64_t>& genome_size, swg_alnstats** out);
// the text side of swg_paf_alnstats (paf_io.cpp; host code only, so that the host translation units link without the device ones)
int swg_paf_stats_prepare(const swg_paf* p, swg_records* rec, std::vector<uint32_t>* col10, const uint32_t** seq_genome);
int swg_paf_stats_finish(const swg_paf* p, const swg_alnstats_result* res /* [2]: ALL, KEPT */, swg_alnstats** const* outs /* [2], NULL = not wanted */);
// the two halves of swg_paf_stats_finish that swg_paf_breadth needs too: genome g's name (trailing '#' kept), and its size in one
// result set (sum of the last-seen lengths of its sequences, read from the lines the set's seq_last names)
void swg_paf_stats_genome_names(const swg_paf* p, std::vector<std::string>* genome_name);
int swg_paf_stats_genome_sizes(const swg_paf* p, const swg_alnstats_result& r, std::vector<uint64_t>* genome_size);
int swg_alnstats_error(int code, const char* fmt, ...);  // sets swg_alnstats_last_error()
extern const char* const SWG_ALNSTATS_FIELD_ERR[6];      // "Invalid query length" ... for columns 2, 3, 4, 7, 10, 11
// the wanted ones of `count` texts as the C ABI hands them out; all or nothing: on a failed allocation every text of this call is freed,
// out_text / out_len of the wanted ones are zeroed and the result is swg_alnstats_error(SWG_ERR_OOM, "out of host memory")
inline int texts_hand_over(const std::string* text, const bool* wanted, int count, char** out_text, uint64_t* out_len) {
  for (int k = 0; k < count; ++k) {
    if (!wanted[k]) continue;
    out_text[k] = text_copy(text[k]);
    out_len[k] = text[k].size();
    if (out_text[k]) continue;
    for (int j = 0; j <= k; ++j) {
      if (!wanted[j]) continue;
      std::free(out_text[j]);
      out_text[j] = nullptr;
      out_len[j] = 0;
    }
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
  return SWG_OK;
}

// ---- breadth (swg_breadth.hip: kernels and seams; alnstats.cpp: the report) ----
struct swg_breadth_result {
  std::vector<swg_breadth_pair> pairs;  // ascending first_record
};
int swg_breadth_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome,
                    const uint8_t* status, swg_breadth_result* all, swg_breadth_result* kept);
// the --breadth report of n_sets result sets (ALL, KEPT) with the genome sizes of each set
int swg_breadth_report(const std::vector<std::string>& genome_name, const swg_breadth_result* res, const std::vector<uint64_t>* genome_size,
                       int n_sets, bool detailed, char** out_text, uint64_t* out_len);

// ---- blocks (swg_blocks.hip: kernels and seams; paf_io.cpp: the text) ----
struct swg_blocks_result {
  std::vector<swg_block> blocks;  // ascending chain number
};
int swg_blocks_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const uint32_t* chain, swg_blocks_result* res);
// the --blocks text: names and lengths from the line of each block's first record
int swg_paf_blocks_text(const swg_paf* p, const std::vector<swg_block>& blocks, char** out_text, uint64_t* out_len);

// ---- components (swg_components.hip: kernels, seams and the text; paf_io.cpp: the lengths) ----
struct swg_components_result {
  std::vector<swg_component> components;  // ascending id
  std::vector<swg_link> links;            // ascending (a, b)
  std::vector<uint32_t> seq_component;    // [n_seq]
  uint64_t cross_links = 0, cross_records = 0, cross_bases = 0;
};
// want_links / want_seq: whether the two long arrays are copied back at all (the counts always are)
int swg_components_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint8_t* status,
                       const swg_component_params* params, bool want_links, bool want_seq, swg_components_result* res);
// per sequence of the handle, the length on the line that mentions it last (target column after query column)
int swg_paf_seq_last_lengths(const swg_paf* p, std::vector<uint32_t>* seq_len);

// ---- lift (swg_lift.hip: kernels and record seams; lift_text.cpp: the BED parser and the texts of swg_paf_lift) ----
// columns of rec, status and regions on the host (on_device = false: staged in the arena) or on the device; req on the host
int swg_lift_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                 swg_lift_request* req);
// ---- base-exact lift (swg_cigar.hip: kernels and record seams; lift_text.cpp: swg_paf_lift_exact;
//      cigar_text.cpp: the tag finder and the row formatter; paf_io.cpp: the handle's lines) ----
// the arrays of the set on the host (on_device = false) or on the device, like the columns; the set structure and req on the host
int swg_lift_exact_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                       const swg_cigar_set* cigars, swg_lift_exact_request* req);
int swg_lift_hit_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                     uint32_t set, uint32_t axes, uint32_t* out, uint64_t capacity, uint64_t* k);
// the value of the last cg:Z: tag of a PAF line (len bytes, with or without its line end), or nullptr; *value_len its length
const char* swg_cigar_tag_find(const char* line, uint64_t len, uint64_t* value_len);
// one line of the exact rows text: dst_name dst_start dst_end label src_name src_start src_end strand axis record aligned matches mode
void swg_lift_exact_row_text(std::string& o, const char* dst_name, const std::string& label, const std::string& src_name, const swg_lift_exact_row& w);
// the handle's text and each record's line in it
void swg_paf_lines_view(const swg_paf* p, const char** text, const uint64_t** rec_off, const uint32_t** rec_len);
// ---- UCSC chain files (swg_ucsc.hip: kernels and record seams; ucsc_text.cpp: the two PAF seams) ----
int swg_ucsc_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint8_t* status, const swg_cigar_set* cigars,
                 swg_ucsc_request* req);
// bytes of CIGAR text per batch when the caller names none: from the memory limit or the free device memory, below 2^32
uint64_t swg_ucsc_default_batch(swg_ctx* ctx);
// `chain score tName tSize + tStart tEnd qName qSize qStrand qStart qEnd id\n` of one row
void swg_ucsc_header_text(std::string& o, const swg_ucsc_chain& ch, const char* ref_name, uint64_t ref_size, const char* oth_name, uint64_t oth_size,
                          uint64_t id);
// first[b] .. first[b + 1]: the entries of batch b -- consecutive entries whose lengths add up to at most batch_bytes, an entry longer
// than that alone; batch_bytes 0: no bound but the call's (fewer than 2^32 bytes).  k == 0: no batch (first = {0}).
void swg_ucsc_plan_batches(const uint64_t* len, uint64_t k, uint64_t batch_bytes, std::vector<uint64_t>* first);
// where the chain file goes: a stream, or a text
struct swg_ucsc_sink {
  std::FILE* file = nullptr;
  std::string* text = nullptr;
  bool failed = false;
  void put(const char* b, size_t n) {
    if (!n) return;
    if (text) text->append(b, n);
    else if (std::fwrite(b, 1, n, file) != n) failed = true;
  }
};
// one batch into the sink: for every row with blocks its header (hdr[j]) and its block lines out of the device's text
void swg_ucsc_splice(swg_ucsc_sink* sink, const swg_ucsc_chain* rows, uint64_t k, const std::string* hdr, const char* text, uint64_t text_bytes);
// ---- lift slices (swg_slice.hip: kernels and record seams; slice_text.cpp: the two PAF seams) ----
int swg_lift_slice_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                       const swg_cigar_set* cigars, swg_lift_slice_request* req);
// The regions of a BED text in line order under the rules of swg_paf_lift, with each one's label (lift_text.cpp: the parser of
// swg_paf_lift against the handle's names); errors name `who` and the line.
int swg_lift_bed_parse(const char* who, const swg_paf* p, const char* bed, uint64_t len, std::vector<swg_lift_region>* regions,
                       std::vector<std::string>* labels);
// first[b] .. first[b + 1]: the regions of batch b -- consecutive regions whose costs add up to at most batch_bytes, a region above
// that alone.  m == 0: no batch (first = {0}).
void swg_slice_plan_batches(const uint64_t* cost, uint64_t m, uint64_t batch_bytes, std::vector<uint64_t>* first);
// one line of the slice PAF: q_name q_len q_start q_end strand t_name t_len t_start t_end col10 block mapq cg:Z:<text> rn:Z:<label>
// ri:i:<record>; line: the record's own line (its columns 2, 7 and 12 are copied), cg / cg_len: the slice's text
void swg_slice_line_text(std::string& o, const char* q_name, const char* t_name, const char* line, uint64_t line_len, const swg_lift_slice& s,
                         const char* cg, const std::string& label);
// ---- variants (swg_variants.hip: kernels and record seams) ----
// where: 0 = everything on the host, 1 = on the device, 2 = the host's with seqs->bases in device memory; entry_usable: host [k] or NULL
int swg_variant_run(swg_ctx* ctx, const swg_records* rec, int where, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                    const swg_cigar_set* cigars, const swg_seq_set* seqs, swg_variant_request* req, uint8_t* entry_usable);
// the bases of the sequences a PAF call names in a device block of their own (src[s] NULL: absent), and its release
int swg_variant_bases_upload(swg_ctx* ctx, const uint8_t* const* src, const uint64_t* len, uint32_t n_seq, uint64_t* offset, uint8_t** d_bases);
void swg_variant_bases_free(swg_ctx* ctx, uint8_t* d_bases);
// order[i] = the index of the i-th variant by the key's low `bits` bits, ties in index order (one stable device sort)
int swg_variant_order(swg_ctx* ctx, const uint64_t* keys, uint64_t n, int bits, uint32_t* order);
// variants_text.cpp: the formatters and the merge of swg_paf_vcf_write, which need neither a handle nor a device
void swg_vcf_escape(std::string& o, const char* s);
void swg_vcf_header_text(std::string& o, const std::vector<std::string>& contig_name, const std::vector<uint64_t>& contig_len, const char* sample);
void swg_vcf_line_text(std::string& o, const char* t_name, const char* q_name, const swg_variant& v, const uint8_t* alleles, bool genotype);
void swg_variants_merge_pairs(std::vector<swg_variant_pair>* total, const swg_variant_pair* add, uint64_t n);
std::string swg_variants_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_variant_pair>& pairs);
// ---- resolved CIGARs (swg_eqx.hip: kernels and record seams; eqx_text.cpp: the two PAF seams) ----
// where: as swg_variant_run
int swg_eqx_run(swg_ctx* ctx, const swg_records* rec, int where, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                swg_eqx_request* req);
// A usable record's line: `line` (len bytes, with or without its line end) with column 10 = matches, column 11 = block and the
// value of its last cg:Z: tag (cg, cg_len: where swg_cigar_tag_find found it) = text[0 .. text_len); a '\n' ends it.
void swg_eqx_line_text(std::string& o, const char* line, uint64_t len, const char* cg, uint64_t cg_len, uint64_t matches, uint64_t block,
                       const char* text, uint64_t text_len);
// ---- alignment blocks as MAF (swg_maf.hip: kernels and record seams; maf_text.cpp: the two PAF seams) ----
// where: as swg_variant_run
int swg_maf_run(swg_ctx* ctx, const swg_records* rec, int where, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                swg_maf_request* req);
// One block as MAF: `a score=<aligned>`, the two `s` lines and an empty line.  line: the record's own line (its columns 2 and 7 are
// the lengths); rows: the block's target row, then its query row, b.columns bytes each.
void swg_maf_block_text(std::string& o, const char* t_name, const char* q_name, const char* line, uint64_t line_len, const swg_maf_block& b,
                        const char* rows);
// ---- differences (swg_diffs.hip: kernels and record seams; diffs_text.cpp: the two PAF seams) ----
int swg_diff_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                 const swg_cigar_set* cigars, swg_diff_request* req);
// `#target t_start t_end query q_start q_end strand kind len left right record\n`, and one row under its two names
void swg_diffs_rows_header(std::string& o);
void swg_diffs_row_text(std::string& o, const char* t_name, const char* q_name, const swg_diff_row& w);
// `add` (ascending by genome pair, as a call returns them) summed into `total` (ascending, and so it stays)
void swg_diffs_merge_pairs(std::vector<swg_diff_pair>* total, const swg_diff_pair* add, uint64_t n);
// header, one line per genome pair, then `#spectrum KIND lo hi count` per non-empty bin of spectrum [4][SWG_DIFF_BINS]
std::string swg_diffs_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_diff_pair>& pairs, const uint64_t* spectrum);
// ---- divergence (swg_divergence.hip: kernels and record seams; divergence_text.cpp: the PAF seam) ----
// vec_rows / vec_seqs: library-owned storage instead of the request's arrays (swg_paf_divergence)
int swg_divergence_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                       const uint8_t* status, const swg_cigar_set* cigars, swg_divergence_request* req, std::vector<swg_divergence_row>* vec_rows,
                       std::vector<swg_divergence_seq>* vec_seqs);
// `#sequence start end n aligned matches mismatches m_columns unaligned inserted mismatch_runs indels\n`, and one row under its name
void swg_divergence_rows_header(std::string& o);
void swg_divergence_row_text(std::string& o, const char* name, const swg_divergence_row& w);
// `#sequence length windows records entries` and the eight sums, and one listed sequence under its name and length
void swg_divergence_summary_header(std::string& o);
void swg_divergence_seq_text(std::string& o, const char* name, uint64_t length, const swg_divergence_seq& s);
// one batch's rows / summaries into the total (first: taken as they are): n, entries and the sums add; false = the keys disagree
bool swg_divergence_merge_rows(std::vector<swg_divergence_row>* total, const std::vector<swg_divergence_row>& add, bool first);
bool swg_divergence_merge_seqs(std::vector<swg_divergence_seq>* total, const std::vector<swg_divergence_seq>& add, bool first);
// ---- transitive lift (swg_lift_closure.hip): swg_lift_run's arguments ----
int swg_lift_closure_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                         swg_closure_request* req);
// hop 0 on the host (lift_text.cpp), all there is without records: validates the regions (returns the lift's bad-input bits, 0 = fine),
// fills req->n and the summaries, and the rows when they fit
uint32_t swg_closure_hop0_host(const swg_lift_region* regions, uint64_t m, uint32_t n_seq, swg_closure_request* req);

// ---- mosaic (swg_mosaic.hip: kernels and seams; mosaic_text.cpp: the two texts of swg_paf_mosaic) ----
// one line per row: sequence start end other_sequence strand record weight other_start other_end (rec: the handle's records,
// with the matches column the device call read)
std::string swg_mosaic_rows_text(const swg_paf* p, const swg_records* rec, const std::vector<swg_mosaic_row>& rows, uint32_t axis, bool by_length);
// `genome other_genome bases`, one line per non-zero entry of share ([G * G], G = genome_name.size()), then `#total <bases>`
std::string swg_mosaic_share_text(const std::vector<std::string>& genome_name, const std::vector<uint64_t>& share, uint64_t bases);

// ---- gaps (swg_gaps.hip: kernels and seams; gaps_text.cpp: the two texts of swg_paf_gaps) ----
// header, then one line per row: query q_lo q_hi target t_lo t_hi kind size chain dq dt left right (rec: the handle's records)
std::string swg_gaps_rows_text(const swg_paf* p, const swg_records* rec, const std::vector<swg_gap_row>& rows);
// header, one line per genome pair (ascending), then `#spectrum KIND lo hi count` per non-empty bin of spectrum [2][SWG_GAPS_BINS]
std::string swg_gaps_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_gap_pair>& pairs, const uint64_t* spectrum);

// ---- place (swg_place.hip: kernels and seams; place_text.cpp: the two texts of swg_paf_place) ----
// header, then one line per row: sequence length partner partner_length orient start end rank bases fwd rev total runner records
// q_lo q_hi t_lo t_hi (seq_len: the lengths the device call read)
std::string swg_place_rows_text(const swg_paf* p, const std::vector<uint32_t>& seq_len, const std::vector<swg_placement>& rows);
// header, then one line per genome pair: genome partner_genome sequences reversed length bases total_bases
std::string swg_place_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_place_pair>& pairs);

// ---- windows (swg_windows.hip: kernels and seams; windows_text.cpp: the two texts of swg_paf_windows) ----
// header, then one line per row: sequence start end n_all depth_all covered_all matches_all n_kept depth_kept covered_kept matches_kept
std::string swg_windows_rows_text(const swg_paf* p, const std::vector<swg_window_row>& rows);
// header, then one line per listed sequence: sequence length windows empty_all empty_kept covered_all covered_kept depth_all depth_kept
// matches_all matches_kept records_all records_kept (seq_len: the lengths the device call read)
std::string swg_windows_summary_text(const swg_paf* p, const std::vector<uint32_t>& seq_len, const std::vector<swg_window_seq>& seqs);

// ---- tree sparsification (tree_filter.cpp: text route and the selection; swg_sparsify.hip: record routes; paf_io.cpp: handles) ----
// one unordered genome pair with its sums; prefix[a] < prefix[b].  The reference accumulates in f64: integer sums below 2^53
// are the same numbers.
struct swg_tree_pair {
  uint32_t a, b;
  double matches, block;
};
constexpr uint64_t SWG_TREE_SUM_LIMIT = uint64_t(1) << 53;
// identity per pair, neighbour ranking (ties: neighbour prefix ascending), SipHash-1-3 random pairs (src/tree_filter.rs:79-160):
// THE selection, for the text route and the record routes alike
void swg_tree_select(const std::vector<std::string>& prefix, const std::vector<swg_tree_pair>& pairs, uint64_t k_nearest,
                     uint64_t k_farthest, double random_fraction, std::vector<uint8_t>* selected);
// the text route's verdicts as a mask over records whose lines start at rec_off[0 .. n) (ascending) of the same text
int swg_tree_text_mask(const char* text, uint64_t len, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                       const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t* n_kept);
// what swg_paf_tree_select / swg_aln_tree_select need of a handle (paf_io.cpp)
struct swg_tree_handle_view {
  const swg_records* rec = nullptr;
  const std::vector<std::string>* prefix_two = nullptr;  // [rec->n_genome_two]
  bool text_route = false;                               // PAF only: the columns are not what the text route reads
  const char* text = nullptr;                            // PAF only
  uint64_t text_len = 0;
  const uint64_t* rec_off = nullptr;
};
void swg_paf_tree_view(const swg_paf* p, swg_tree_handle_view* v);
void swg_aln_tree_view(const swg_aln* a, swg_tree_handle_view* v);
#endif

// ---- --joblist (fasta_io.cpp, swg_mash.hip, mash_host.cpp) ----
// detect_file_type's FASTA test over text already loaded
bool swg_fasta_text_is_fasta(const char* p, size_t n);
// the sketch of swg_mash_sketch, handed over contig by contig: emit(user, contig, ascending values, count), in contig order
int swg_mash_sketch_each(swg_ctx* ctx, const uint8_t* seq, const uint64_t* offsets, uint64_t n_seq, int k, uint64_t s,
                         void (*emit)(void*, uint64_t, const uint64_t*, uint64_t), void* user, double* timing_ms);
#endif
