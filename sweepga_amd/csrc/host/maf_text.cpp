// swg_paf_maf_write / swg_paf_maf_text: the records of an open PAF as MAF blocks, the two rows of every block
// gathered through the CIGAR on the device.  The handle's sequence names are matched to the FASTA records by exact name as
// swg_paf_vcf_write does it, the bases of the sequences the set names go to the device once per call, host threads find the last
// cg:Z: tag of every record of the set, and the records go to the device in batches (swg_ucsc_plan_batches) of bounded cost: an
// entry's text length plus (q_end - q_start) + (t_end - t_start), a bound on its alignment columns.  At 2 bytes per column that also
// bounds the output, so a batch is ONE device pass with the bound as text capacity.  One function body, two sinks.  The block
// formatter needs neither a handle nor a device: tests/native/maf_text_check.cpp builds this file on its own.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"
#include "threads.h"

namespace {

// tab-separated field `want` (from 0) of a line of len bytes, without the line end; false when the line has fewer fields
bool line_field(const char* line, uint64_t len, int want, const char** at, uint64_t* n) {
  while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) --len;
  uint64_t pos = 0;
  for (int f = 0;; ++f) {
    const void* tab = std::memchr(line + pos, '\t', len - pos);
    const uint64_t end = tab ? (uint64_t)((const char*)tab - line) : len;
    if (f == want) {
      *at = line + pos, *n = end - pos;
      return true;
    }
    if (!tab) return false;
    pos = end + 1;
  }
}

// the decimal value of field `want` (a record of the handle has its lengths there: digits only), 0 when there is none
uint64_t field_value(const char* line, uint64_t len, int want) {
  const char* at;
  uint64_t n, v = 0;
  if (!line_field(line, len, want, &at, &n)) return 0;
  for (uint64_t i = 0; i < n && (unsigned)(at[i] - '0') < 10u; ++i) v = v * 10 + (uint64_t)(at[i] - '0');
  return v;
}

}  // namespace

void swg_maf_block_text(std::string& o, const char* t_name, const char* q_name, const char* line, uint64_t line_len, const swg_maf_block& b,
                        const char* rows) {
  const uint64_t t_len = field_value(line, line_len, 6), q_len = field_value(line, line_len, 1);
  const bool minus = (b.flags & SWG_MAF_MINUS) != 0;
  o += "a score=";
  append_u64(o, b.aligned, '\n');
  o += "s ";
  o += t_name;
  o += ' ';
  append_u64(o, b.t_start, ' ');
  append_u64(o, b.t_bases, ' ');
  o += "+ ";
  append_u64(o, t_len, ' ');
  o.append(rows, b.columns);
  o += "\ns ";
  o += q_name;
  o += ' ';
  append_u64(o, minus ? q_len - b.q_start - b.q_bases : (uint64_t)b.q_start, ' ');  // MAF counts a '-' row from the reverse strand's start
  append_u64(o, b.q_bases, ' ');
  o += minus ? "- " : "+ ";
  append_u64(o, q_len, ' ');
  o.append(rows + b.columns, b.columns);
  o += "\n\n";
}

namespace {

const char MAF_HEADER[] = "##maf version=1\n";

int host_threads(uint64_t items) {
  return (int)std::min<uint64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), items / 4096 + 1);
}

// what needs neither a device nor a file; 0 = fine
int refusal(const char* who, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_maf_options* opts) {
  if (!opts) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL options", who);
  if (opts->set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (opts->reserved != 0) return swg_alnstats_error(SWG_ERR_INVALID, "%s: reserved must be 0", who);
  if (opts->set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (!fasta) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL sequences: the rows are the FASTA records' bases", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: blocks over 64-bit columns are not supported", who);
  return SWG_OK;
}

struct bases_guard {  // the device block of the bases lives across the batches
  swg_ctx* ctx;
  uint8_t* d = nullptr;
  ~bases_guard() { swg_variant_bases_free(ctx, d); }
};

int paf_maf(const char* who, swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_maf_options* opts, swg_ucsc_sink* sink,
            swg_maf_counts* counts) {
  const int refused = refusal(who, p, status, fasta, opts);
  if (refused != SWG_OK) return refused;
  const swg_records* rec = swg_paf_records(p);
  std::vector<uint32_t> sel;  // the records of the set, ascending
  for (uint64_t i = 0; i < rec->n; ++i)
    if (opts->set == SWG_IV_ALL || status[i] != 0) sel.push_back((uint32_t)i);
  const uint64_t k = sel.size();
  swg_maf_counts c{};
  c.records = k;
  if (k && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
  sink->put(MAF_HEADER, sizeof(MAF_HEADER) - 1);
  c.file_bytes = sizeof(MAF_HEADER) - 1;
  if (k) {
    const uint32_t n_seq = rec->n_seq;
    // the sequences the set names, matched by exact name; one whose PAF length differs from the FASTA's is absent
    std::vector<uint32_t> seq_len;
    const int lens = swg_paf_seq_last_lengths(p, &seq_len);
    if (lens != SWG_OK) return lens;
    std::vector<uint8_t> named(n_seq, 0);
    for (uint64_t j = 0; j < k; ++j) named[rec->q_id[sel[j]]] = named[rec->t_id[sel[j]]] = 1;
    std::unordered_map<std::string, uint64_t> by_name;
    const uint64_t n_fasta = swg_fasta_num_records(fasta);
    const uint64_t* f_off = swg_fasta_offsets(fasta);
    const uint8_t* f_bases = swg_fasta_bases(fasta);
    for (uint64_t i = n_fasta; i-- > 0;) by_name[swg_fasta_name(fasta, i)] = i;  // (of two records with one name the first)
    std::vector<const uint8_t*> src(n_seq, nullptr);
    std::vector<uint64_t> src_len(n_seq, 0), seq_offset(n_seq + 1, 0);
    for (uint32_t s = 0; s < n_seq; ++s) {
      if (!named[s]) continue;
      const auto at = by_name.find(swg_paf_sequence_name(p, s));
      if (at == by_name.end()) continue;
      const uint64_t len = f_off[at->second + 1] - f_off[at->second];
      if (len != seq_len[s]) {
        ++c.length_mismatch;
        continue;
      }
      src[s] = f_bases + f_off[at->second], src_len[s] = len;
    }
    bases_guard bases{ctx};
    int rc = swg_variant_bases_upload(ctx, src.data(), src_len.data(), n_seq, seq_offset.data(), &bases.d);
    if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    const swg_seq_set seqs{seq_offset.data(), bases.d, n_seq, 0};

    const char* paf_text;
    const uint64_t* rec_off;
    const uint32_t* rec_len;
    swg_paf_lines_view(p, &paf_text, &rec_off, &rec_len);
    std::vector<const char*> at(k);
    std::vector<uint64_t> len(k), cost(k), breakable(k);
    const int threads = host_threads(k);
    const bool split = opts->split_gap != 0;
    swg_host::run(threads, [&](int t) {
      for (uint64_t j = k * t / threads; j < k * (t + 1) / threads; ++j) {
        at[j] = swg_cigar_tag_find(paf_text + rec_off[sel[j]], rec_len[sel[j]], &len[j]);
        uint64_t b = 0;  // an entry has at most one block more than it has I, D and N ops
        if (split && at[j])
          for (uint64_t q = 0; q < len[j]; ++q) b += at[j][q] == 'I' || at[j][q] == 'D' || at[j][q] == 'N';
        breakable[j] = b;
      }
    });
    for (uint64_t j = 0; j < k; ++j) {
      c.untagged += at[j] == nullptr;
      if (len[j] >> 32) return swg_alnstats_error(SWG_ERR_RANGE, "%s: the CIGAR of record %llu has 2^32 bytes or more", who, (unsigned long long)sel[j]);
      const uint32_t r = sel[j];
      const uint64_t lq = rec->q_end[r] >= rec->q_start[r] ? rec->q_end[r] - rec->q_start[r] : 0, lt = rec->t_end[r] >= rec->t_start[r] ? rec->t_end[r] - rec->t_start[r] : 0;
      cost[j] = len[j] + lq + lt;  // (a usable entry has no more alignment columns than lq + lt: its advances are the record's lengths)
    }
    std::vector<uint64_t> first;
    // (below 2^31: the output's bound is at most twice the cost)
    swg_ucsc_plan_batches(cost.data(), k, std::min<uint64_t>(opts->batch_bytes ? opts->batch_bytes : swg_ucsc_default_batch(ctx), (uint64_t(1) << 31) - 1), &first);
    std::vector<uint32_t> col[6], local;
    std::vector<uint8_t> strand;
    std::vector<uint64_t> offset;
    std::string cigar_text;
    std::vector<swg_maf_block> blocks;
    std::vector<char> out_text;
    const uint32_t* const from[6] = {rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end};
    for (size_t b = 0; b + 1 < first.size(); ++b) {
      const uint64_t a = first[b], kb = first[b + 1] - a;
      for (auto& v : col) v.resize(kb);
      strand.resize(kb), local.resize(kb), offset.assign(kb + 1, 0);
      uint64_t bound = 0, block_bound = kb;  // of the batch's output text: two bytes per alignment column; of its blocks
      for (uint64_t j = 0; j < kb; ++j) {
        const uint32_t r = sel[a + j];
        for (int f = 0; f < 6; ++f) col[f][j] = from[f][r];
        strand[j] = rec->strand[r], local[j] = (uint32_t)j;
        offset[j + 1] = offset[j] + len[a + j];
        bound += 2 * (cost[a + j] - len[a + j]);
        block_bound += breakable[a + j];
      }
      if (offset[kb] >> 32)
        return swg_alnstats_error(SWG_ERR_RANGE, "%s: a batch of 2^32 bytes or more: record %llu alone is too large for one call", who, (unsigned long long)sel[a]);
      cigar_text.resize(offset[kb]);
      const int bt = host_threads(kb);
      swg_host::run(bt, [&](int t) {
        for (uint64_t j = kb * t / bt; j < kb * (t + 1) / bt; ++j)
          if (at[a + j]) std::memcpy(&cigar_text[offset[j]], at[a + j], len[a + j]);
      });
      swg_records part{};
      part.n = kb, part.n_seq = n_seq;
      part.q_id = col[0].data(), part.t_id = col[1].data(), part.q_start = col[2].data(), part.q_end = col[3].data();
      part.t_start = col[4].data(), part.t_end = col[5].data(), part.strand = strand.data();
      const swg_cigar_set cigars{local.data(), offset.data(), cigar_text.data(), kb};
      if (blocks.size() < block_bound) blocks.resize(block_bound);
      if (out_text.size() < bound) out_text.resize(bound);
      swg_maf_request req{};
      req.set = SWG_IV_ALL, req.split_gap = opts->split_gap;
      req.block_capacity = blocks.size(), req.blocks = blocks.data();
      req.text_capacity = out_text.size(), req.text = out_text.data();
      rc = swg_maf_run(ctx, &part, 2, nullptr, &cigars, &seqs, &req);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      if (req.text_bytes > req.text_capacity || req.n_blocks > req.block_capacity)
        return swg_alnstats_error(SWG_ERR_INVALID, "%s: a batch's output is larger than its bound", who);  // (never)
      const uint64_t nb = req.n_blocks;
      const int ft = host_threads(nb);
      std::vector<std::string> text(ft);
      swg_host::run(ft, [&](int t) {
        for (uint64_t i = nb * t / ft; i < nb * (t + 1) / ft; ++i) {
          const swg_maf_block& blk = blocks[i];
          const uint32_t r = sel[a + blk.entry];
          swg_maf_block_text(text[t], swg_paf_sequence_name(p, rec->t_id[r]), swg_paf_sequence_name(p, rec->q_id[r]), paf_text + rec_off[r], rec_len[r], blk,
                             out_text.data() + blk.text_first);
        }
      });
      for (const std::string& s : text) sink->put(s.data(), s.size()), c.file_bytes += s.size();
      c.usable += req.usable, c.bad += req.cigar_bad, c.no_sequence += req.no_sequence, c.out_of_sequence += req.out_of_sequence;
      c.blocks += req.n_blocks, c.gap_only += req.gap_only, c.breakers += req.breakers, c.skipped_t += req.skipped_t, c.skipped_q += req.skipped_q;
      c.columns += req.columns, c.aligned += req.aligned;
      ++c.batches;
    }
  }
  if (sink->failed) return swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
  if (counts) *counts = c;
  return SWG_OK;
}

}  // namespace

extern "C" int swg_paf_maf_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_maf_options* opts,
                                 const char* out_path, swg_maf_counts* counts) {
  static const char* const who = "swg_paf_maf_write";
  if (!p || !out_path) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  try {
    // (the refusals come before a file is touched; the checks that need no device are the function body's own first step)
    const int refused = refusal(who, p, status, fasta, opts);
    if (refused != SWG_OK) return refused;
    std::FILE* f = std::fopen(out_path, "wb");
    if (!f) return swg_alnstats_error(SWG_ERR_INVALID, "%s: cannot open %s: %s", who, out_path, std::strerror(errno));
    swg_ucsc_sink sink;
    sink.file = f;
    int rc = paf_maf(who, ctx, p, status, fasta, opts, &sink, counts);
    if (std::fclose(f) != 0 && rc == SWG_OK) rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    return rc;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_paf_maf_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_fasta* fasta, const swg_maf_options* opts,
                                swg_maf_counts* counts, char** text, uint64_t* len) {
  static const char* const who = "swg_paf_maf_text";
  if (text) *text = nullptr;
  if (len) *len = 0;
  if (!p || !text || !len) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  try {
    std::string out;
    swg_ucsc_sink sink;
    sink.text = &out;
    const int rc = paf_maf(who, ctx, p, status, fasta, opts, &sink, counts);
    if (rc != SWG_OK) return rc;
    const bool wanted[1] = {true};
    return texts_hand_over(&out, wanted, 1, text, len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
