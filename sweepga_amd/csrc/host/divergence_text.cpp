// swg_paf_divergence: the divergence track of an open PAF.  Host threads find the last cg:Z: tag of every
// record of the set, the set goes to the device in batches of bounded CIGAR text (swg_ucsc_plan_batches; swg_divergence.hip builds
// the rows and the summary of ALL records under that batch's CIGAR set), and the rows and summaries are added up here across the
// batches: the window table is the same in every batch, only the entry-derived fields differ.  The formatters and the merge need
// neither a handle nor a device: tests/native/divergence_text_check.cpp builds this file on its own.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"
#include "threads.h"

void swg_divergence_rows_header(std::string& o) {
  o += "#sequence\tstart\tend\tn\taligned\tmatches\tmismatches\tm_columns\tunaligned\tinserted\tmismatch_runs\tindels\n";
}

void swg_divergence_row_text(std::string& o, const char* name, const swg_divergence_row& w) {
  o += name;
  o += '\t';
  append_u64(o, w.start, '\t');
  append_u64(o, w.end, '\t');
  append_u64(o, w.n, '\t');
  const uint64_t* v = &w.aligned;
  for (int f = 0; f < 8; ++f) append_u64(o, v[f], f == 7 ? '\n' : '\t');
}

void swg_divergence_summary_header(std::string& o) {
  o += "#sequence\tlength\twindows\trecords\tentries\taligned\tmatches\tmismatches\tm_columns\tunaligned\tinserted\tmismatch_runs\tindels\n";
}

void swg_divergence_seq_text(std::string& o, const char* name, uint64_t length, const swg_divergence_seq& s) {
  o += name;
  o += '\t';
  append_u64(o, length, '\t');
  append_u64(o, s.windows, '\t');
  append_u64(o, s.records, '\t');
  append_u64(o, s.entries, '\t');
  const uint64_t* v = &s.aligned;
  for (int f = 0; f < 8; ++f) append_u64(o, v[f], f == 7 ? '\n' : '\t');
}

// One batch's rows into the total: the first batch is taken as it is; a later one must have the same windows, and its n and eight
// sums add.  false: the keys disagree (the batches did not see the same records).
bool swg_divergence_merge_rows(std::vector<swg_divergence_row>* total, const std::vector<swg_divergence_row>& add, bool first) {
  if (first) {
    *total = add;
    return true;
  }
  if (total->size() != add.size()) return false;
  for (size_t i = 0; i < add.size(); ++i) {
    swg_divergence_row& t = (*total)[i];
    const swg_divergence_row& a = add[i];
    if (t.seq != a.seq || t.start != a.start || t.end != a.end) return false;
    t.n += a.n;
    uint64_t* d = &t.aligned;
    const uint64_t* v = &a.aligned;
    for (int f = 0; f < 8; ++f) d[f] += v[f];
  }
  return true;
}

// The same for the summaries: seq, windows and records are the same in every batch; entries and the eight sums add.
bool swg_divergence_merge_seqs(std::vector<swg_divergence_seq>* total, const std::vector<swg_divergence_seq>& add, bool first) {
  if (first) {
    *total = add;
    return true;
  }
  if (total->size() != add.size()) return false;
  for (size_t i = 0; i < add.size(); ++i) {
    swg_divergence_seq& t = (*total)[i];
    const swg_divergence_seq& a = add[i];
    if (t.seq != a.seq || t.windows != a.windows || t.records != a.records) return false;
    uint64_t* d = &t.entries;
    const uint64_t* v = &a.entries;
    for (int f = 0; f < 9; ++f) d[f] += v[f];
  }
  return true;
}

namespace {

int host_threads(uint64_t items) {
  return (int)std::min<uint64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), items / 4096 + 1);
}

}  // namespace

extern "C" int swg_paf_divergence(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t axis, uint32_t window,
                                  const char* other_genome, uint64_t batch_bytes, char** out_text, uint64_t* out_len, swg_divergence_counts* counts) {
  static const char* const who = "swg_paf_divergence";
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  const bool wanted[2] = {out_text[0] != nullptr, out_text[1] != nullptr};
  out_text[0] = out_text[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "%s: neither text is asked for", who);
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (axis > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: axis is 0 (query) or 1 (target)", who);
  if (window == 0) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the window size is at least 1", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))  // (before the context is looked at)
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: the divergence of 64-bit columns is not supported", who);
  try {
    const uint64_t n = swg_paf_records(p)->n;
    std::vector<uint32_t> sel;  // the records of the set, ascending
    for (uint64_t i = 0; i < n; ++i)
      if (set == SWG_IV_ALL || status[i] != 0) sel.push_back((uint32_t)i);
    const uint64_t k = sel.size();
    swg_divergence_counts c{};
    c.records = k;
    std::vector<swg_divergence_row> rows, total_rows;
    std::vector<swg_divergence_seq> seqs, total_seqs;
    std::vector<uint32_t> seq_len;
    if (k) {  // (a PAF without records of the set has no rows and gives the headers whatever the genome's name)
      std::vector<std::string> gname;
      swg_paf_stats_genome_names(p, &gname);
      uint32_t other = SWG_WINDOWS_ANY;
      if (other_genome) {
        const std::string name(other_genome);
        for (size_t g = 0; g < gname.size() && other == SWG_WINDOWS_ANY; ++g)
          if (gname[g] == name || gname[g] == name + "#") other = (uint32_t)g;
        if (other == SWG_WINDOWS_ANY) return swg_alnstats_error(SWG_ERR_INVALID, "%s: unknown genome '%s'", who, other_genome);
      }
      if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
      const swg_records& rec = *swg_paf_records(p);
      const uint32_t* seq_genome = rec.seq_genome_last;  // (the last-'#' map of swg_paf_windows)
      int rc = swg_paf_seq_last_lengths(p, &seq_len);
      if (rc != SWG_OK) return rc;
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
      std::vector<uint64_t> offset;
      std::string cigar_text;
      for (size_t b = 0; b + 1 < first.size(); ++b) {
        const uint64_t a = first[b], kb = first[b + 1] - a;
        offset.assign(kb + 1, 0);
        for (uint64_t j = 0; j < kb; ++j) offset[j + 1] = offset[j] + len[a + j];
        cigar_text.resize(offset[kb]);
        const int bt = host_threads(kb);
        swg_host::run(bt, [&](int t) {
          for (uint64_t j = kb * t / bt; j < kb * (t + 1) / bt; ++j)
            if (at[a + j]) std::memcpy(&cigar_text[offset[j]], at[a + j], len[a + j]);
        });
        const swg_cigar_set cigars{sel.data() + a, offset.data(), cigar_text.data(), kb};
        swg_divergence_request req{};
        req.set = set, req.axis = axis, req.window = window, req.other_genome = other;
        req.want = SWG_DIVERGENCE_ROWS | SWG_DIVERGENCE_SUMMARY;  // (the counts name both, whichever text is asked for)
        rc = swg_divergence_run(ctx, &rec, false, seq_len.data(), seq_genome, rec.n_genome_last, status, &cigars, &req, &rows, &seqs);
        if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
        if (!swg_divergence_merge_rows(&total_rows, rows, b == 0) || !swg_divergence_merge_seqs(&total_seqs, seqs, b == 0))
          return swg_alnstats_error(SWG_ERR_INVALID, "%s: the window tables of two batches disagree", who);
        c.usable += req.usable, c.bad += req.cigar_bad;
        ++c.batches;
      }
      c.windows = total_rows.size(), c.seqs = total_seqs.size();
    }
    std::string text[2];
    if (wanted[0]) {
      swg_divergence_rows_header(text[0]);
      for (const swg_divergence_row& w : total_rows) swg_divergence_row_text(text[0], swg_paf_sequence_name(p, w.seq), w);
    }
    if (wanted[1]) {
      swg_divergence_summary_header(text[1]);
      for (const swg_divergence_seq& s : total_seqs) swg_divergence_seq_text(text[1], swg_paf_sequence_name(p, s.seq), seq_len[s.seq], s);
    }
    const int handed = texts_hand_over(text, wanted, 2, out_text, out_len);
    if (handed != SWG_OK) return handed;
    if (counts) *counts = c;
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
