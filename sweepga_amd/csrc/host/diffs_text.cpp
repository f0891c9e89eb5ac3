// swg_paf_diffs_write / swg_paf_diffs_text: the difference list of an open PAF.  Host threads find the last
// cg:Z: tag of every record of the set, the records go to the device in batches of bounded CIGAR text (swg_ucsc_plan_batches; swg_diffs.hip
// builds the rows and the sums), the rows are formatted here batch by batch -- they carry the names -- and the pair sums and the
// spectrum are added up across the batches.  One function body, two sinks.  The formatters and the merge need neither a handle nor a
// device: tests/native/diffs_text_check.cpp builds this file on its own.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"
#include "threads.h"

void swg_diffs_rows_header(std::string& o) { o += "#target\tt_start\tt_end\tquery\tq_start\tq_end\tstrand\tkind\tlen\tleft\tright\trecord\n"; }

void swg_diffs_row_text(std::string& o, const char* t_name, const char* q_name, const swg_diff_row& w) {
  const uint32_t kind = w.kind_flags & 0xffu;
  o += t_name;
  o += '\t';
  append_u64(o, w.t_start, '\t');
  append_u64(o, w.t_end, '\t');
  o += q_name;
  o += '\t';
  append_u64(o, w.q_start, '\t');
  append_u64(o, w.q_end, '\t');
  o += w.kind_flags & SWG_DIFF_MINUS ? "-\t" : "+\t";
  o += kind == SWG_DIFF_SNP ? "SNP\t" : kind == SWG_DIFF_INS ? "INS\t" : kind == SWG_DIFF_DEL ? "DEL\t" : "SKIP\t";
  append_u64(o, kind == SWG_DIFF_INS ? w.q_end - w.q_start : w.t_end - w.t_start, '\t');
  append_u64(o, w.left, '\t');
  append_u64(o, w.right, '\t');
  append_u64(o, w.record, '\n');
}

void swg_diffs_merge_pairs(std::vector<swg_diff_pair>* total, const swg_diff_pair* add, uint64_t n) {
  auto before = [](const swg_diff_pair& a, const swg_diff_pair& b) { return a.q_genome != b.q_genome ? a.q_genome < b.q_genome : a.t_genome < b.t_genome; };
  std::vector<swg_diff_pair> out;
  out.reserve(total->size() + n);
  size_t i = 0;
  uint64_t j = 0;
  while (i < total->size() || j < n) {
    if (j == n || (i < total->size() && before((*total)[i], add[j]))) {
      out.push_back((*total)[i++]);
    } else if (i == total->size() || before(add[j], (*total)[i])) {
      out.push_back(add[j++]);
    } else {  // the same genome pair: the twelve sums behind the two ids
      swg_diff_pair s = (*total)[i++];
      const uint64_t* v = &add[j++].entries;
      uint64_t* d = &s.entries;
      for (int f = 0; f < 12; ++f) d[f] += v[f];
      out.push_back(s);
    }
  }
  total->swap(out);
}

// One line per genome pair, then the non-empty bins of the spectrum with their inclusive bounds (bin b: lengths of b bits).
std::string swg_diffs_summary_text(const std::vector<std::string>& genome_name, const std::vector<swg_diff_pair>& pairs, const uint64_t* spectrum) {
  static const char* const KIND[4] = {"SNP\t", "INS\t", "DEL\t", "SKIP\t"};
  std::string o = "#query_genome\ttarget_genome\tentries\taligned\teq\tm_columns\tsnp_runs\tsnp_bases\tins\tins_bases\tdel\tdel_bases\tskip\tskip_bases\n";
  for (const swg_diff_pair& g : pairs) {
    o += genome_name[g.q_genome];
    o += '\t';
    o += genome_name[g.t_genome];
    o += '\t';
    const uint64_t* v = &g.entries;
    for (int f = 0; f < 12; ++f) append_u64(o, v[f], f == 11 ? '\n' : '\t');
  }
  for (int kind = 0; kind < 4; ++kind)
    for (int b = 0; b < SWG_DIFF_BINS; ++b) {
      const uint64_t count = spectrum[kind * SWG_DIFF_BINS + b];
      if (!count) continue;
      o += "#spectrum\t";
      o += KIND[kind];
      append_u64(o, b ? uint64_t(1) << (b - 1) : 0, '\t');
      append_u64(o, b ? (uint64_t(1) << b) - 1 : 0, '\t');
      append_u64(o, count, '\n');
    }
  return o;
}

namespace {

int host_threads(uint64_t items) {
  return (int)std::min<uint64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), items / 4096 + 1);
}

// what needs neither a device nor a file; 0 = fine
int refusal(const char* who, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t kinds) {
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (kinds == 0 || kinds > 15) return swg_alnstats_error(SWG_ERR_INVALID, "%s: kinds names nothing, or a bit beyond the four", who);
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: differences from 64-bit columns are not supported", who);
  return SWG_OK;
}

// rows: nullptr = the rows are counted and not built; summary: nullptr = not wanted
int paf_diffs(const char* who, swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t kinds, uint32_t min_indel,
              uint64_t batch_bytes, swg_ucsc_sink* rows_sink, std::string* summary, swg_diff_counts* counts) {
  const int refused = refusal(who, p, status, set, kinds);
  if (refused != SWG_OK) return refused;
  const swg_records* rec = swg_paf_records(p);
  std::vector<uint32_t> sel;  // the records of the set, ascending
  for (uint64_t i = 0; i < rec->n; ++i)
    if (set == SWG_IV_ALL || status[i] != 0) sel.push_back((uint32_t)i);
  const uint64_t k = sel.size();
  swg_diff_counts c{};
  c.records = k;
  if (k) {
    if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
    const char* paf_text;
    const uint64_t* rec_off;
    const uint32_t* rec_len;
    swg_paf_lines_view(p, &paf_text, &rec_off, &rec_len);
    std::vector<const char*> at(k);
    std::vector<uint64_t> len(k);
    const int threads = host_threads(k);
    swg_host::run(threads, [&](int t) {
      for (uint64_t j = k * t / threads; j < k * (t + 1) / threads; ++j) at[j] = swg_cigar_tag_find(paf_text + rec_off[sel[j]], rec_len[sel[j]], &len[j]);
    });
    for (uint64_t j = 0; j < k; ++j) {
      c.untagged += at[j] == nullptr;
      if (len[j] >> 32) return swg_alnstats_error(SWG_ERR_RANGE, "%s: the CIGAR of record %llu has 2^32 bytes or more", who, (unsigned long long)sel[j]);
    }
    std::vector<uint64_t> first;
    swg_ucsc_plan_batches(len.data(), k, batch_bytes ? batch_bytes : swg_ucsc_default_batch(ctx), &first);
    const uint32_t G = rec->n_genome_two;
    std::vector<uint32_t> col[6], local;
    std::vector<uint8_t> strand;
    std::vector<uint64_t> offset;
    std::string cigar_text, lines;
    std::vector<swg_diff_row> rows;
    std::vector<swg_diff_pair> pairs, total;
    std::vector<std::string> part_text;
    uint64_t spectrum[4 * SWG_DIFF_BINS], sum_spectrum[4 * SWG_DIFF_BINS] = {0};
    const uint32_t* const src[6] = {rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end};
    if (rows_sink) {
      swg_diffs_rows_header(lines);
      rows_sink->put(lines.data(), lines.size());
    }
    for (size_t b = 0; b + 1 < first.size(); ++b) {
      const uint64_t a = first[b], kb = first[b + 1] - a;
      // the batch's records as a record set of their own: what is staged follows the batch, not the file
      for (auto& v : col) v.resize(kb);
      strand.resize(kb), local.resize(kb), offset.assign(kb + 1, 0);
      for (uint64_t j = 0; j < kb; ++j) {
        const uint32_t r = sel[a + j];
        for (int f = 0; f < 6; ++f) col[f][j] = src[f][r];
        strand[j] = rec->strand[r], local[j] = (uint32_t)j;
        offset[j + 1] = offset[j] + len[a + j];
      }
      cigar_text.resize(offset[kb]);
      const int bt = host_threads(kb);
      swg_host::run(bt, [&](int t) {
        for (uint64_t j = kb * t / bt; j < kb * (t + 1) / bt; ++j)
          if (at[a + j]) std::memcpy(&cigar_text[offset[j]], at[a + j], len[a + j]);
      });
      swg_records part{};
      part.n = kb, part.n_seq = rec->n_seq;
      part.q_id = col[0].data(), part.t_id = col[1].data(), part.q_start = col[2].data(), part.q_end = col[3].data();
      part.t_start = col[4].data(), part.t_end = col[5].data(), part.strand = strand.data();
      const swg_cigar_set cigars{local.data(), offset.data(), cigar_text.data(), kb};
      pairs.resize((size_t)std::min<uint64_t>((uint64_t)G * G, kb));
      if (rows_sink && rows.size() < offset[kb] / 64 + 4096) rows.resize(offset[kb] / 64 + 4096);  // a first guess; a second call when there are more
      swg_diff_request req{};
      req.set = SWG_IV_ALL, req.kinds = kinds, req.min_indel = min_indel;
      req.row_capacity = rows_sink ? rows.size() : 0, req.rows = rows_sink ? rows.data() : nullptr;
      req.pair_capacity = pairs.size(), req.pairs = pairs.data();
      req.spectrum = spectrum;
      int rc = swg_diff_run(ctx, &part, false, rec->seq_genome_two, G, nullptr, &cigars, &req);
      if (rc == SWG_OK && rows_sink && req.n_rows > req.row_capacity) {
        rows.resize(req.n_rows);
        req.row_capacity = rows.size(), req.rows = rows.data();
        rc = swg_diff_run(ctx, &part, false, rec->seq_genome_two, G, nullptr, &cigars, &req);
      }
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      if (rows_sink && req.n_rows) {
        const uint64_t nr = req.n_rows;
        const int rt = host_threads(nr);
        part_text.assign(rt, std::string());
        swg_host::run(rt, [&](int t) {
          for (uint64_t i = nr * t / rt; i < nr * (t + 1) / rt; ++i) {
            const uint32_t r = sel[a + rows[i].record];
            swg_diff_row w = rows[i];
            w.record = r;  // (the call numbered the batch's records: the file's number goes out)
            swg_diffs_row_text(part_text[t], swg_paf_sequence_name(p, rec->t_id[r]), swg_paf_sequence_name(p, rec->q_id[r]), w);
          }
        });
        for (const std::string& s : part_text) rows_sink->put(s.data(), s.size());
        if (rows_sink->failed) return swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
      }
      swg_diffs_merge_pairs(&total, pairs.data(), req.n_pairs);
      for (int s = 0; s < 4 * SWG_DIFF_BINS; ++s) sum_spectrum[s] += spectrum[s];
      c.usable += req.usable, c.bad += req.cigar_bad, c.rows += req.n_rows;
      ++c.batches;
    }
    for (const swg_diff_pair& g : total) {
      c.snp_runs += g.snp_runs, c.snp_bases += g.snp_bases, c.n_ins += g.n_ins, c.ins_bases += g.ins_bases;
      c.n_del += g.n_del, c.del_bases += g.del_bases, c.n_skip += g.n_skip, c.skip_bases += g.skip_bases, c.m_columns += g.m_columns;
    }
    if (summary) {
      std::vector<std::string> gname(G);
      for (uint32_t g = 0; g < G; ++g) gname[g] = swg_paf_genome_two_prefix(p, g);
      *summary = swg_diffs_summary_text(gname, total, sum_spectrum);
    }
  }
  if (counts) *counts = c;
  return SWG_OK;
}

}  // namespace

extern "C" int swg_paf_diffs_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t kinds, uint32_t min_indel,
                                   uint64_t batch_bytes, const char* rows_path, const char* summary_path, swg_diff_counts* counts) {
  static const char* const who = "swg_paf_diffs_write";
  if (!p || (!rows_path && !summary_path)) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument, or neither file is asked for", who);
  try {
    // (the refusals come before a file is touched; the checks that need no device are the function body's own first step)
    const int refused = refusal(who, p, status, set, kinds);
    if (refused != SWG_OK) return refused;
    std::FILE* f = nullptr;
    if (rows_path && !(f = std::fopen(rows_path, "wb")))
      return swg_alnstats_error(SWG_ERR_INVALID, "%s: cannot open %s: %s", who, rows_path, std::strerror(errno));
    std::FILE* g = nullptr;
    if (summary_path && !(g = std::fopen(summary_path, "wb"))) {
      const int e = errno;
      if (f) std::fclose(f);
      return swg_alnstats_error(SWG_ERR_INVALID, "%s: cannot open %s: %s", who, summary_path, std::strerror(e));
    }
    swg_ucsc_sink sink;
    sink.file = f;
    std::string summary;
    int rc = paf_diffs(who, ctx, p, status, set, kinds, min_indel, batch_bytes, f ? &sink : nullptr, g ? &summary : nullptr, counts);
    if (g && rc == SWG_OK && !summary.empty() && std::fwrite(summary.data(), 1, summary.size(), g) != summary.size())
      rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    if (f && std::fclose(f) != 0 && rc == SWG_OK) rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    if (g && std::fclose(g) != 0 && rc == SWG_OK) rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    return rc;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_paf_diffs_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t kinds, uint32_t min_indel,
                                  uint64_t batch_bytes, swg_diff_counts* counts, char** rows_text, uint64_t* rows_len, char** summary_text,
                                  uint64_t* summary_len) {
  static const char* const who = "swg_paf_diffs_text";
  if (rows_text) *rows_text = nullptr;
  if (rows_len) *rows_len = 0;
  if (summary_text) *summary_text = nullptr;
  if (summary_len) *summary_len = 0;
  if (!p || (!rows_text && !summary_text) || (rows_text && !rows_len) || (summary_text && !summary_len))
    return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument, or neither text is asked for", who);
  try {
    std::string text[2];
    swg_ucsc_sink sink;
    sink.text = &text[0];
    const int rc = paf_diffs(who, ctx, p, status, set, kinds, min_indel, batch_bytes, rows_text ? &sink : nullptr, summary_text ? &text[1] : nullptr, counts);
    if (rc != SWG_OK) return rc;
    const bool wanted[2] = {rows_text != nullptr, summary_text != nullptr};
    char* out[2] = {nullptr, nullptr};
    uint64_t len[2] = {0, 0};
    const int handed = texts_hand_over(text, wanted, 2, out, len);
    if (handed != SWG_OK) return handed;
    if (rows_text) *rows_text = out[0], *rows_len = len[0];
    if (summary_text) *summary_text = out[1], *summary_len = len[1];
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
