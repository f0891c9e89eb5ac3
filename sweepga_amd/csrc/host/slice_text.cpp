// swg_paf_lift_paf_write / swg_paf_lift_paf_text: BED regions lifted through an open PAF, every slice as a PAF
// line with its own coordinates and its sliced cg:Z:.  One plain lift gives the hits per region and with them each region's cost; the
// BED goes to the device in batches of consecutive regions of bounded cost (swg_slice.hip cuts the slices and copies their text), and
// the lines -- they carry the names, the lengths and the mapping quality of the record's own line -- are written here.  One function
// body, two sinks.  The line writer and the batch planner need neither a handle nor a device: tests/native/slice_text_check.cpp builds
// this file on its own.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

void swg_slice_plan_batches(const uint64_t* cost, uint64_t m, uint64_t batch_bytes, std::vector<uint64_t>* first) {
  const uint64_t top = 0xffffffffull;  // a call writes fewer than 2^32 bytes
  const uint64_t bound = batch_bytes && batch_bytes < top ? batch_bytes : top;
  first->assign(1, 0);
  uint64_t held = 0;
  for (uint64_t r = 0; r < m; ++r) {
    if (r > first->back() && held + cost[r] > bound) {
      first->push_back(r);
      held = 0;
    }
    held += cost[r];
  }
  if (m) first->push_back(m);
}

namespace {

// tab-separated field `want` (from 0) of a line of len bytes: its bytes, without the line end; false when the line has fewer fields
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

void append_field(std::string& o, const char* line, uint64_t len, int want) {
  const char* at;
  uint64_t n;
  if (line_field(line, len, want, &at, &n)) o.append(at, n);
  else o += '0';  // (a record of the handle has twelve columns: never)
  o += '\t';
}

}  // namespace

void swg_slice_line_text(std::string& o, const char* q_name, const char* t_name, const char* line, uint64_t line_len, const swg_lift_slice& s,
                         const char* cg, const std::string& label) {
  o += q_name;
  o += '\t';
  append_field(o, line, line_len, 1);
  append_u64(o, s.q_start, '\t');
  append_u64(o, s.q_end, '\t');
  o += s.flags & SWG_LIFT_MINUS ? "-\t" : "+\t";
  o += t_name;
  o += '\t';
  append_field(o, line, line_len, 6);
  append_u64(o, s.t_start, '\t');
  append_u64(o, s.t_end, '\t');
  append_u64(o, s.flags & SWG_SLICE_HAS_EQ ? s.matches : s.aligned, '\t');
  append_u64(o, s.block, '\t');
  append_field(o, line, line_len, 11);
  o += "cg:Z:";
  o.append(cg, s.text_len);
  o += "\trn:Z:";
  o += label;
  o += "\tri:i:";
  append_u64(o, s.record, '\n');
}

namespace {

// the refusals that need neither the BED nor a device; SWG_OK when there is none
int refusal(const char* who, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set, uint32_t axes) {
  if (!p || (!bed && bed_len)) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (axes == 0 || axes >> 2) return swg_alnstats_error(SWG_ERR_INVALID, "%s: axes names nothing, or a bit beyond the two", who);
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept rows need a status column", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: a lift through 64-bit columns is not supported", who);
  return SWG_OK;
}

struct Tag {
  const char* at;
  uint64_t len;
};

int paf_lift_paf(const char* who, swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set,
                 uint32_t axes, uint32_t min_aligned, uint64_t batch_bytes, swg_ucsc_sink* sink, swg_lift_paf_counts* counts) {
  const int refused = refusal(who, p, status, bed, bed_len, set, axes);
  if (refused != SWG_OK) return refused;
  std::vector<swg_lift_region> regions;
  std::vector<std::string> labels;
  const int parsed = swg_lift_bed_parse(who, p, bed, bed_len, &regions, &labels);
  if (parsed != SWG_OK) return parsed;
  const swg_records* rec = swg_paf_records(p);
  const uint64_t m = regions.size();
  swg_lift_paf_counts c{};
  if (m && rec->n) {
    if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
    // the hits per region: one plain lift, its rows in region order
    std::vector<swg_lift_row> rows(std::max<uint64_t>(4 * m, uint64_t(1) << 16));  // a first guess; a second call when there are more
    swg_lift_request plain{};
    plain.set = set, plain.axes = axes;
    plain.capacity = rows.size(), plain.rows = rows.data();
    int rc = swg_lift_run(ctx, rec, false, status, regions.data(), m, &plain);
    if (rc == SWG_OK && plain.n > plain.capacity) {
      rows.resize(plain.n);
      plain.capacity = rows.size(), plain.rows = rows.data();
      rc = swg_lift_run(ctx, rec, false, status, regions.data(), m, &plain);
    }
    if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    rows.resize(plain.n);
    const char* paf_text;
    const uint64_t* rec_off;
    const uint32_t* rec_len;
    swg_paf_lines_view(p, &paf_text, &rec_off, &rec_len);
    std::unordered_map<uint32_t, Tag> tags;  // the last cg:Z: tag of every record that is hit
    std::vector<uint64_t> cost(m, 0), region_rows(m, 0);
    for (const swg_lift_row& w : rows) {
      auto it = tags.find(w.record);
      if (it == tags.end()) {
        Tag t{nullptr, 0};
        t.at = swg_cigar_tag_find(paf_text + rec_off[w.record], rec_len[w.record], &t.len);
        if (!t.at) t.len = 0;
        it = tags.emplace(w.record, t).first;
      }
      cost[w.region] += it->second.len + 24;
      ++region_rows[w.region];
    }
    for (uint64_t r = 0; r < m; ++r)
      if (cost[r] >> 32) return swg_alnstats_error(SWG_ERR_RANGE, "%s: the CIGARs under region %llu have 2^32 bytes or more", who, (unsigned long long)r);
    std::vector<uint64_t> first;
    swg_slice_plan_batches(cost.data(), m, batch_bytes ? batch_bytes : swg_ucsc_default_batch(ctx), &first);
    std::vector<uint32_t> hit;
    std::vector<uint64_t> offset;
    std::vector<uint8_t> state;
    std::vector<swg_lift_slice> slices;
    std::string cigar_text, slice_text, lines;
    for (size_t b = 0; b + 1 < first.size(); ++b) {
      const uint64_t a = first[b], mb = first[b + 1] - a;
      uint64_t batch_rows = 0, batch_cost = 0;
      for (uint64_t r = a; r < a + mb; ++r) batch_rows += region_rows[r], batch_cost += cost[r];
      c.rows += batch_rows;
      if (!batch_rows) continue;  // no hit: no line
      hit.resize(batch_rows);  // (at most one distinct record per row)
      uint64_t k = 0;
      rc = swg_lift_hit_run(ctx, rec, false, status, regions.data() + a, mb, set, axes, hit.data(), hit.size(), &k);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      hit.resize(k);
      offset.assign(k + 1, 0);
      for (uint64_t j = 0; j < k; ++j) offset[j + 1] = offset[j] + tags.at(hit[j]).len;
      cigar_text.resize(offset[k]);
      for (uint64_t j = 0; j < k; ++j)
        if (const Tag& t = tags.at(hit[j]); t.len) std::memcpy(&cigar_text[offset[j]], t.at, t.len);
      const swg_cigar_set cigars{hit.data(), offset.data(), cigar_text.data(), k};
      slices.resize(batch_rows), state.resize(k), slice_text.resize(batch_cost);  // (the cost bounds the text: a slice is no longer than its entry)
      swg_lift_slice_request req{};
      req.set = set, req.axes = axes, req.min_aligned = min_aligned;
      req.slice_capacity = slices.size(), req.slices = slices.data();
      req.text_capacity = slice_text.size(), req.text = &slice_text[0];
      req.state = state.data();
      rc = swg_lift_slice_run(ctx, rec, false, status, regions.data() + a, mb, &cigars, &req);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      if (req.n_slices > req.slice_capacity || req.text_bytes > req.text_capacity)
        return swg_alnstats_error(SWG_ERR_INVALID, "%s: a batch gave more slices or text than its hits allow", who);  // (never)
      lines.clear();
      for (uint64_t s = 0; s < req.n_slices; ++s) {
        const swg_lift_slice& w = slices[s];
        swg_slice_line_text(lines, swg_paf_sequence_name(p, rec->q_id[w.record]), swg_paf_sequence_name(p, rec->t_id[w.record]),
                            paf_text + rec_off[w.record], rec_len[w.record], w, slice_text.data() + w.text_first, labels[a + w.region]);
      }
      sink->put(lines.data(), lines.size());
      if (sink->failed) return swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
      c.slices += req.n_slices, c.interp += req.n_interp, c.empty += req.n_empty, c.too_short += req.n_short;
      c.hits += k, c.bad += req.cigar_bad;
      ++c.batches;
    }
  }
  if (counts) *counts = c;
  return SWG_OK;
}

}  // namespace

extern "C" int swg_paf_lift_paf_write(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set,
                                      uint32_t axes, uint32_t min_aligned, uint64_t batch_bytes, const char* out_path, swg_lift_paf_counts* counts) {
  static const char* const who = "swg_paf_lift_paf_write";
  if (!out_path) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  try {
    const int refused = refusal(who, p, status, bed, bed_len, set, axes);  // (before the file is touched)
    if (refused != SWG_OK) return refused;
    {
      std::vector<swg_lift_region> regions;
      std::vector<std::string> labels;
      const int parsed = swg_lift_bed_parse(who, p, bed, bed_len, &regions, &labels);
      if (parsed != SWG_OK) return parsed;
    }
    std::FILE* f = std::fopen(out_path, "wb");
    if (!f) return swg_alnstats_error(SWG_ERR_INVALID, "%s: cannot open %s: %s", who, out_path, std::strerror(errno));
    swg_ucsc_sink sink;
    sink.file = f;
    int rc = paf_lift_paf(who, ctx, p, status, bed, bed_len, set, axes, min_aligned, batch_bytes, &sink, counts);
    if (std::fclose(f) != 0 && rc == SWG_OK) rc = swg_alnstats_error(SWG_ERR_INVALID, "%s: write failed: %s", who, std::strerror(errno));
    return rc;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_paf_lift_paf_text(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set,
                                     uint32_t axes, uint32_t min_aligned, uint64_t batch_bytes, swg_lift_paf_counts* counts, char** text,
                                     uint64_t* len) {
  static const char* const who = "swg_paf_lift_paf_text";
  if (!text || !len) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  *text = nullptr, *len = 0;
  try {
    std::string out;
    swg_ucsc_sink sink;
    sink.text = &out;
    const int rc = paf_lift_paf(who, ctx, p, status, bed, bed_len, set, axes, min_aligned, batch_bytes, &sink, counts);
    if (rc != SWG_OK) return rc;
    if (!(*text = text_copy(out))) return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
    *len = out.size();
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
