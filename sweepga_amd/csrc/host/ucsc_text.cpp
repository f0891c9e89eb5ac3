// swg_paf_ucsc_chain_write / swg_paf_ucsc_chain_text: the chain file of an open PAF.  Host threads find the
// last cg:Z: tag of every record of the set, the records go to the device in batches of bounded CIGAR text (swg_ucsc.hip builds the
// blocks and formats their lines), and the header lines -- they carry the names -- are formatted here and spliced with the device's
// text.  One function body, two sinks.  The header formatter, the batch planner and the splice need neither a handle nor a device:
// tests/native/ucsc_text_check.cpp builds this file on its own.
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

void swg_ucsc_header_text(std::string& o, const swg_ucsc_chain& ch, const char* ref_name, uint64_t ref_size, const char* oth_name, uint64_t oth_size,
                          uint64_t id) {
  o += "chain ";
  append_u64(o, ch.score, ' ');
  o += ref_name;
  o += ' ';
  append_u64(o, ref_size, ' ');
  o += "+ ";
  append_u64(o, ch.ref_start, ' ');
  append_u64(o, ch.ref_end, ' ');
  o += oth_name;
  o += ' ';
  append_u64(o, oth_size, ' ');
  o += ch.flags & SWG_UCSC_MINUS ? "- " : "+ ";
  append_u64(o, ch.oth_start, ' ');
  append_u64(o, ch.oth_end, ' ');
  append_u64(o, id, '\n');
}

void swg_ucsc_plan_batches(const uint64_t* len, uint64_t k, uint64_t batch_bytes, std::vector<uint64_t>* first) {
  const uint64_t top = 0xffffffffull;  // a call takes fewer than 2^32 bytes
  const uint64_t bound = batch_bytes && batch_bytes < top ? batch_bytes : top;
  first->assign(1, 0);
  uint64_t held = 0;
  for (uint64_t j = 0; j < k; ++j) {
    if (j > first->back() && held + len[j] > bound) {
      first->push_back(j);
      held = 0;
    }
    held += len[j];
  }
  if (k) first->push_back(k);
}

void swg_ucsc_splice(swg_ucsc_sink* sink, const swg_ucsc_chain* rows, uint64_t k, const std::string* hdr, const char* text, uint64_t text_bytes) {
  uint64_t prev = k;  // the last row with blocks whose end is not yet known
  for (uint64_t j = 0; j <= k; ++j) {
    if (j < k && rows[j].n_blocks == 0) continue;
    const uint64_t at = j < k ? rows[j].text_first : text_bytes;
    if (prev < k) sink->put(text + rows[prev].text_first, (size_t)(at - rows[prev].text_first));
    if (j < k) sink->put(hdr[j].data(), hdr[j].size());
    prev = j;
  }
}

namespace {

int host_threads(uint64_t items) {
  return (int)std::min<uint64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), items / 4096 + 1);
}

int paf_ucsc(const char* who, swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t from, uint64_t batch_bytes,
             swg_ucsc_sink* sink, swg_ucsc_counts* counts) {
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (from > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: from must be SWG_UCSC_FROM_TARGET or SWG_UCSC_FROM_QUERY", who);
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: chains from 64-bit columns are not supported", who);
  const swg_records* rec = swg_paf_records(p);
  std::vector<uint32_t> sel;  // the records of the set, ascending
  for (uint64_t i = 0; i < rec->n; ++i)
    if (set == SWG_IV_ALL || status[i] != 0) sel.push_back((uint32_t)i);
  const uint64_t k = sel.size();
  swg_ucsc_counts c{};
  c.records = k;
  if (k) {
    if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
    std::vector<uint32_t> seq_len;
    const int lens = swg_paf_seq_last_lengths(p, &seq_len);
    if (lens != SWG_OK) return lens;
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
    std::vector<uint32_t> col[6], local;
    std::vector<uint8_t> strand, state;
    std::vector<uint64_t> offset;
    std::string cigar_text, device_text;
    std::vector<swg_ucsc_chain> rows;
    std::vector<swg_ucsc_block> blocks;  // (not asked for: the text is what a file needs)
    std::vector<std::string> hdr;
    std::vector<uint64_t> id;
    const uint32_t* const src[6] = {rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end};
    uint64_t next_id = 1;
    for (size_t b = 0; b + 1 < first.size(); ++b) {
      const uint64_t a = first[b], kb = first[b + 1] - a;
      // the batch's records as a record set of their own: what is staged follows the batch, not the file
      for (auto& v : col) v.resize(kb);
      strand.resize(kb), local.resize(kb), state.resize(kb), offset.assign(kb + 1, 0);
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
      rows.resize(kb);
      if (device_text.size() < 2 * offset[kb] + 4096) device_text.resize(2 * offset[kb] + 4096);  // a first guess; a second call when there is more
      swg_ucsc_request req{};
      req.set = SWG_IV_ALL, req.from = from;
      req.chain_capacity = kb, req.chains = rows.data();
      req.text_capacity = device_text.size(), req.text = &device_text[0];
      req.state = state.data();
      int rc = swg_ucsc_run(ctx, &part, false, seq_len.data(), nullptr, &cigars, &req);
      if (rc == SWG_OK && req.text_bytes > req.text_capacity) {
        device_text.resize(req.text_bytes);
        req.text_capacity = device_text.size(), req.text = &device_text[0];
        rc = swg_ucsc_run(ctx, &part, false, seq_len.data(), nullptr, &cigars, &req);
      }
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      id.resize(kb);
      for (uint64_t j = 0; j < kb; ++j) id[j] = rows[j].n_blocks ? next_id++ : 0;
      hdr.resize(kb);
      swg_host::run(bt, [&](int t) {
        for (uint64_t j = kb * t / bt; j < kb * (t + 1) / bt; ++j) {
          hdr[j].clear();
          if (!rows[j].n_blocks) continue;
          const uint32_t r = sel[a + j];
          const uint32_t ref = from == SWG_UCSC_FROM_QUERY ? rec->q_id[r] : rec->t_id[r], oth = from == SWG_UCSC_FROM_QUERY ? rec->t_id[r] : rec->q_id[r];
          swg_ucsc_header_text(hdr[j], rows[j], swg_paf_sequence_name(p, ref), seq_len[ref], swg_paf_sequence_name(p, oth), seq_len[oth], id[j]);
        }
      });
      swg_ucsc_splice(sink, rows.data(), kb, hdr.data(), device_text.data(), req.text_bytes);
      if (sink->failed) return swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
      c.chains += req.n_chains, c.bad += req.cigar_bad, c.beyond += req.beyond, c.empty += req.empty_chains, c.blocks += req.n_blocks;
      ++c.batches;
    }
  }
  if (counts) *counts = c;
  return SWG_OK;
}

}  // namespace

extern "C" int swg_paf_ucsc_chain_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t from, const char* out_path,
                                        uint64_t batch_bytes, swg_ucsc_counts* counts) {
  static const char* const who = "swg_paf_ucsc_chain_write";
  if (!p || !out_path) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  try {
    // (the refusals come before the file is touched: a first pass into no sink would cost the device work twice, so the checks that
    // need no device are repeated here)
    if (set > 1 || from > 1 || (set == SWG_IV_KEPT && !status) || swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0)) {
      swg_ucsc_sink none;
      return paf_ucsc(who, ctx, p, status, set, from, batch_bytes, &none, counts);
    }
    std::FILE* f = std::fopen(out_path, "wb");
    if (!f) return swg_alnstats_error(SWG_ERR_INVALID, "%s: cannot open %s: %s", who, out_path, std::strerror(errno));
    swg_ucsc_sink sink;
    sink.file = f;
    int rc = paf_ucsc(who, ctx, p, status, set, from, batch_bytes, &sink, counts);
    if (std::fclose(f) != 0 && rc == SWG_OK) rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    return rc;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_paf_ucsc_chain_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t set, uint32_t from, uint64_t batch_bytes,
                                       swg_ucsc_counts* counts, char** text, uint64_t* len) {
  static const char* const who = "swg_paf_ucsc_chain_text";
  if (!p || !text || !len) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  *text = nullptr, *len = 0;
  try {
    std::string out;
    swg_ucsc_sink sink;
    sink.text = &out;
    const int rc = paf_ucsc(who, ctx, p, status, set, from, batch_bytes, &sink, counts);
    if (rc != SWG_OK) return rc;
    if (!(*text = text_copy(out))) return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
    *len = out.size();
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
