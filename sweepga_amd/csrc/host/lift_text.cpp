// swg_paf_lift: BED regions parsed on the host, lifted through an open PAF by one device call
// (swg_lift.hip), and the two texts -- rows and per-region summary -- written with the handle's names.  swg_paf_lift_exact (section
// 30) is the same through the CIGARs of the hit records' lines (swg_cigar.hip, cigar_text.cpp).  swg_paf_lift_closure
// (section 24) is the same around the transitive lift (swg_lift_closure.hip), with hop 0 on the host for a PAF without records.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"
#include "threads.h"

namespace {

struct BedRegion {
  std::string name, label;
};

bool starts_with(std::string_view s, const char* prefix) { return s.substr(0, std::strlen(prefix)) == prefix; }

// decimal digits only, a value below 2^32
bool parse_u32(std::string_view t, uint32_t* out) {
  if (t.empty() || t.size() > 10) return false;
  uint64_t v = 0;
  for (char ch : t) {
    if (ch < '0' || ch > '9') return false;
    v = v * 10 + (uint64_t)(ch - '0');
  }
  if (v >> 32) return false;
  *out = (uint32_t)v;
  return true;
}

// The regions of a BED text in line order.  Tab-separated; name, start, end required, a non-empty fourth column is the label (default
// name:start-end), further columns are ignored; empty lines and lines starting with '#', "track" or "browser" are skipped.
int parse_bed(const char* who, const char* bed, uint64_t len, const std::unordered_map<std::string_view, uint32_t>& ids,
              std::vector<swg_lift_region>* regions, std::vector<BedRegion>* text) {
  uint64_t line_no = 0;
  for (uint64_t pos = 0; pos < len;) {
    const void* nl = std::memchr(bed + pos, '\n', len - pos);
    const uint64_t end = nl ? (uint64_t)((const char*)nl - bed) : len;
    std::string_view line(bed + pos, end - pos);
    pos = end + 1;
    ++line_no;
    if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
    if (line.empty() || line[0] == '#' || starts_with(line, "track") || starts_with(line, "browser")) continue;
    std::string_view col[4];
    int n_col = 0;
    for (size_t at = 0; n_col < 4;) {
      const size_t tab = line.find('\t', at);
      col[n_col++] = line.substr(at, tab == std::string_view::npos ? std::string_view::npos : tab - at);
      if (tab == std::string_view::npos) break;
      at = tab + 1;
    }
    const unsigned long long ln = line_no;
    if (n_col < 3) return swg_alnstats_error(SWG_ERR_INVALID, "%s: BED line %llu: fewer than three tab-separated columns", who, ln);
    if (col[0].empty()) return swg_alnstats_error(SWG_ERR_INVALID, "%s: BED line %llu: empty sequence name", who, ln);
    swg_lift_region g{0, 0, 0, 0};
    if (!parse_u32(col[1], &g.start)) return swg_alnstats_error(SWG_ERR_INVALID, "%s: BED line %llu: start is not a number below 2^32", who, ln);
    if (!parse_u32(col[2], &g.end)) return swg_alnstats_error(SWG_ERR_INVALID, "%s: BED line %llu: end is not a number below 2^32", who, ln);
    if (g.start > g.end) return swg_alnstats_error(SWG_ERR_INVALID, "%s: BED line %llu: start > end", who, ln);
    const auto it = ids.find(col[0]);
    g.seq = it == ids.end() ? UINT32_MAX : it->second;
    BedRegion b;
    b.name.assign(col[0]);
    if (n_col == 4 && !col[3].empty()) b.label.assign(col[3]);
    else b.label = b.name + ':' + std::to_string(g.start) + '-' + std::to_string(g.end);
    regions->push_back(g);
    text->push_back(std::move(b));
  }
  return SWG_OK;
}

// the counts of the calling thread's last successful swg_paf_lift_exact: records hit, state 0, bad, without a tag
thread_local uint64_t exact_counts[4] = {0, 0, 0, 0};

// The CIGAR set of the records `hit` (ascending) of an open PAF: the last cg:Z: tag of each one's line, found by host threads over
// rec_off / rec_len, laid end to end; a line without the tag gives an empty entry.  Returns the entries without a tag.
uint64_t gather_cigars(const swg_paf* p, const std::vector<uint32_t>& hit, std::vector<uint64_t>* offset, std::string* text) {
  const char* paf_text;
  const uint64_t* rec_off;
  const uint32_t* rec_len;
  swg_paf_lines_view(p, &paf_text, &rec_off, &rec_len);
  const uint64_t k = hit.size();
  std::vector<const char*> at(k);
  offset->assign(k + 1, 0);
  const int threads = (int)std::min<uint64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), k / 4096 + 1);
  swg_host::run(threads, [&](int t) {
    for (uint64_t j = k * t / threads; j < k * (t + 1) / threads; ++j)
      at[j] = swg_cigar_tag_find(paf_text + rec_off[hit[j]], rec_len[hit[j]], &(*offset)[j + 1]);
  });
  uint64_t untagged = 0;
  for (uint64_t j = 0; j < k; ++j) {
    untagged += at[j] == nullptr;
    (*offset)[j + 1] += (*offset)[j];
  }
  text->resize((*offset)[k]);
  swg_host::run(threads, [&](int t) {
    for (uint64_t j = k * t / threads; j < k * (t + 1) / threads; ++j)
      if (at[j]) std::memcpy(&(*text)[(*offset)[j]], at[j], (*offset)[j + 1] - (*offset)[j]);
  });
  return untagged;
}

// swg_paf_lift and swg_paf_lift_exact: one contract, one BED parser, one summary text; `exact` routes the rows through the CIGARs
int paf_lift(const char* who, bool exact, swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set,
             uint32_t axes, char** out_text, uint64_t* out_len) {
  if (!p || !out_text || !out_len || (!bed && bed_len)) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  const bool wanted[2] = {out_text[0] != nullptr, out_text[1] != nullptr};
  out_text[0] = out_text[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "%s: neither text is asked for", who);
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (axes == 0 || axes >> 2) return swg_alnstats_error(SWG_ERR_INVALID, "%s: axes names nothing, or a bit beyond the two", who);
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept rows need a status column", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: a lift through 64-bit columns is not supported", who);
  try {
    const uint32_t n_names = swg_paf_num_sequences(p);
    std::unordered_map<std::string_view, uint32_t> ids;
    ids.reserve(n_names);
    for (uint32_t s = 0; s < n_names; ++s) ids.emplace(swg_paf_sequence_name(p, s), s);
    std::vector<swg_lift_region> regions;
    std::vector<BedRegion> bed_text;
    const int parsed = parse_bed(who, bed, bed_len, ids, &regions, &bed_text);
    if (parsed != SWG_OK) return parsed;
    const swg_records* rec = swg_paf_records(p);
    const uint64_t m = regions.size();
    std::string text[2];
    text[1] = "label\tsequence\tstart\tend\tall_q\tall_t\tkept_q\tkept_t\tstate\n";
    uint64_t counts[4] = {0, 0, 0, 0};
    if (m && rec->n) {
      if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
      std::vector<swg_lift_summary> summary(m);
      if (!exact) {
        std::vector<swg_lift_row> rows;
        swg_lift_request req{};
        req.set = set, req.axes = axes;
        req.summary = summary.data();
        if (wanted[0]) {  // a first guess at the rows; a second call when there are more
          rows.resize(std::max<uint64_t>(4 * m, uint64_t(1) << 16));
          req.capacity = rows.size(), req.rows = rows.data();
        }
        int rc = swg_lift_run(ctx, rec, false, status, regions.data(), m, &req);
        if (rc == SWG_OK && wanted[0] && req.n > req.capacity) {
          rows.resize(req.n);
          req.capacity = rows.size(), req.rows = rows.data();
          rc = swg_lift_run(ctx, rec, false, status, regions.data(), m, &req);
        }
        if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
        if (wanted[0]) {
          for (uint64_t k = 0; k < req.n; ++k) {
            const swg_lift_row& w = rows[k];
            const uint32_t ax = w.flags >> 1 & 1u;
            std::string& o = text[0];
            o += swg_paf_sequence_name(p, w.dst_seq);
            o += '\t';
            append_u64(o, w.dst_start, '\t');
            append_u64(o, w.dst_end, '\t');
            o += bed_text[w.region].label;
            o += '\t';
            o += bed_text[w.region].name;
            o += '\t';
            append_u64(o, w.src_start, '\t');
            append_u64(o, w.src_end, '\t');
            o += w.flags & SWG_LIFT_MINUS ? "-\t" : "+\t";
            o += ax ? "t\t" : "q\t";
            append_u64(o, w.record, '\n');
          }
        }
      } else {
        // the hit records, their CIGARs from the lines, then the exact call: the lift's index is built once for the list and once
        // for the rows
        std::vector<uint32_t> hit(std::max<uint64_t>(4 * m, uint64_t(1) << 16));
        uint64_t k = 0;
        int rc = swg_lift_hit_run(ctx, rec, false, status, regions.data(), m, set, axes, hit.data(), hit.size(), &k);
        if (rc == SWG_OK && k > hit.size()) {
          hit.resize(k);
          rc = swg_lift_hit_run(ctx, rec, false, status, regions.data(), m, set, axes, hit.data(), hit.size(), &k);
        }
        if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
        hit.resize(k);
        std::vector<uint64_t> offset;
        std::string cigar_text;
        counts[3] = gather_cigars(p, hit, &offset, &cigar_text);
        const swg_cigar_set cigars{hit.data(), offset.data(), cigar_text.data(), k};
        std::vector<swg_lift_exact_row> rows;
        swg_lift_exact_request req{};
        req.set = set, req.axes = axes;
        req.summary = summary.data();
        std::vector<uint8_t> state(k);
        req.state = k ? state.data() : nullptr;
        if (wanted[0]) {
          rows.resize(std::max<uint64_t>(4 * m, uint64_t(1) << 16));
          req.capacity = rows.size(), req.rows = rows.data();
        }
        rc = swg_lift_exact_run(ctx, rec, false, status, regions.data(), m, &cigars, &req);
        if (rc == SWG_OK && wanted[0] && req.n > req.capacity) {
          rows.resize(req.n);
          req.capacity = rows.size(), req.rows = rows.data();
          rc = swg_lift_exact_run(ctx, rec, false, status, regions.data(), m, &cigars, &req);
        }
        if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
        counts[0] = k, counts[1] = (uint64_t)std::count(state.begin(), state.end(), uint8_t(0)), counts[2] = req.cigar_bad;
        if (wanted[0])
          for (uint64_t r = 0; r < req.n; ++r) {
            const swg_lift_exact_row& w = rows[r];
            swg_lift_exact_row_text(text[0], swg_paf_sequence_name(p, w.dst_seq), bed_text[w.region].label, bed_text[w.region].name, w);
          }
      }
      if (wanted[1]) {
        for (uint64_t r = 0; r < m; ++r) {
          const swg_lift_summary& s = summary[r];
          std::string& o = text[1];
          o += bed_text[r].label;
          o += '\t';
          o += bed_text[r].name;
          o += '\t';
          append_u64(o, regions[r].start, '\t');
          append_u64(o, regions[r].end, '\t');
          append_u64(o, s.hits[0][0], '\t');
          append_u64(o, s.hits[0][1], '\t');
          if (status) {
            append_u64(o, s.hits[1][0], '\t');
            append_u64(o, s.hits[1][1], '\t');
          } else {
            o += "-\t-\t";
          }
          const bool any_all = s.hits[0][0] + (uint64_t)s.hits[0][1] > 0, any_kept = s.hits[1][0] + (uint64_t)s.hits[1][1] > 0;
          o += regions[r].seq == UINT32_MAX ? "unknown\n" : !any_all ? "none\n" : !status ? "all\n" : any_kept ? "kept\n" : "lost\n";
        }
      }
    }
    const int rc = texts_hand_over(text, wanted, 2, out_text, out_len);
    if (rc == SWG_OK && exact) std::memcpy(exact_counts, counts, sizeof counts);
    return rc;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

int swg_lift_bed_parse(const char* who, const swg_paf* p, const char* bed, uint64_t len, std::vector<swg_lift_region>* regions,
                       std::vector<std::string>* labels) {
  const uint32_t n_names = swg_paf_num_sequences(p);
  std::unordered_map<std::string_view, uint32_t> ids;
  ids.reserve(n_names);
  for (uint32_t s = 0; s < n_names; ++s) ids.emplace(swg_paf_sequence_name(p, s), s);
  std::vector<BedRegion> text;
  const int rc = parse_bed(who, bed, len, ids, regions, &text);
  if (rc != SWG_OK) return rc;
  for (BedRegion& b : text) labels->push_back(std::move(b.label));
  return SWG_OK;
}

extern "C" int swg_paf_lift(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set, uint32_t axes,
                            char** out_text, uint64_t* out_len) {
  return paf_lift("swg_paf_lift", false, ctx, p, status, bed, bed_len, set, axes, out_text, out_len);
}

extern "C" int swg_paf_lift_exact(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set,
                                  uint32_t axes, char** out_text, uint64_t* out_len) {
  return paf_lift("swg_paf_lift_exact", true, ctx, p, status, bed, bed_len, set, axes, out_text, out_len);
}

extern "C" void swg_paf_lift_exact_counts(uint64_t out[4]) { std::memcpy(out, exact_counts, sizeof exact_counts); }

uint32_t swg_closure_hop0_host(const swg_lift_region* regions, uint64_t m, uint32_t n_seq, swg_closure_request* req) {
  uint64_t n = 0;
  for (uint64_t r = 0; r < m; ++r) {
    const swg_lift_region& g = regions[r];
    const uint32_t bad = (g.reserved != 0 ? 2u : 0u) | (g.start > g.end ? 4u : 0u) | (g.seq >= n_seq && g.seq != UINT32_MAX ? 8u : 0u);
    if (bad) return bad;
    n += g.seq != UINT32_MAX && g.start < g.end;
  }
  const bool fetch = req->rows && n <= req->capacity;
  uint64_t k = 0;
  for (uint64_t r = 0; r < m; ++r) {
    const swg_lift_region& g = regions[r];
    const bool piece = g.seq != UINT32_MAX && g.start < g.end;
    if (req->summary) req->summary[r] = piece ? swg_closure_summary{(uint64_t)g.end - g.start, 1, 1, 0, 0} : swg_closure_summary{0, 0, 0, 0, 0};
    if (piece && fetch) req->rows[k++] = swg_closure_row{(uint32_t)r, g.seq, g.start, g.end, 0, 0};
  }
  req->n = n;
  req->hops_run = 0;
  req->projections = req->candidates[0] = req->candidates[1] = 0;
  return 0;
}

extern "C" int swg_paf_lift_closure(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const char* bed, uint64_t bed_len, uint32_t set,
                                    uint32_t axes, uint32_t max_hops, uint32_t min_len, char** out_text, uint64_t* out_len) {
  static const char* const who = "swg_paf_lift_closure";
  if (!p || !out_text || !out_len || (!bed && bed_len)) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL argument", who);
  const bool wanted[2] = {out_text[0] != nullptr, out_text[1] != nullptr};
  out_text[0] = out_text[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "%s: neither text is asked for", who);
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (axes == 0 || axes >> 2) return swg_alnstats_error(SWG_ERR_INVALID, "%s: axes names nothing, or a bit beyond the two", who);
  if (max_hops == 0 || max_hops > 65535u) return swg_alnstats_error(SWG_ERR_INVALID, "%s: max_hops must be 1 .. 65535", who);
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "%s: the file has a value >= 2^32, its columns are rebased: a lift through 64-bit columns is not supported", who);
  try {
    const uint32_t n_names = swg_paf_num_sequences(p);
    std::unordered_map<std::string_view, uint32_t> ids;
    ids.reserve(n_names);
    for (uint32_t s = 0; s < n_names; ++s) ids.emplace(swg_paf_sequence_name(p, s), s);
    std::vector<swg_lift_region> regions;
    std::vector<BedRegion> bed_text;
    const int parsed = parse_bed(who, bed, bed_len, ids, &regions, &bed_text);
    if (parsed != SWG_OK) return parsed;
    const swg_records* rec = swg_paf_records(p);
    const uint64_t m = regions.size();
    std::string text[2];
    text[1] = "label\tsequence\tstart\tend\tpieces\tsequences\tgenomes\tbases\thops\tstate\n";
    if (m) {
      std::vector<swg_closure_summary> summary(m);
      std::vector<swg_closure_row> rows(std::max<uint64_t>(4 * m, uint64_t(1) << 16));  // a first guess; a second call when there are more
      swg_closure_request req{};
      req.set = set, req.axes = axes, req.max_hops = max_hops, req.min_len = min_len;
      req.summary = summary.data();
      req.capacity = rows.size(), req.rows = rows.data();  // (the genomes column needs the rows even when their text is not asked for)
      auto run = [&]() -> int {
        if (rec->n == 0) return swg_closure_hop0_host(regions.data(), m, rec->n_seq, &req) ? SWG_ERR_INVALID : SWG_OK;  // (the parser's regions are sound)
        if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "%s: NULL context", who);
        const int rc = swg_lift_closure_run(ctx, rec, false, status, regions.data(), m, &req);
        return rc == SWG_OK ? rc : swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      };
      int rc = run();
      if (rc == SWG_OK && req.n > req.capacity) {
        rows.resize(req.n);
        req.capacity = rows.size(), req.rows = rows.data();
        rc = run();
      }
      if (rc != SWG_OK) return rc;
      std::vector<uint32_t> genomes(m, 0);
      {  // rows are ordered by region: the distinct genome prefixes of each run
        std::unordered_set<std::string_view> seen;
        for (uint64_t k = 0; k < req.n; ++k) {
          const swg_closure_row& w = rows[k];
          if (k && rows[k - 1].region != w.region) seen.clear();
          const std::string_view name(swg_paf_sequence_name(p, w.seq));
          const size_t hash = name.rfind('#');
          genomes[w.region] += seen.insert(hash == std::string_view::npos ? name : name.substr(0, hash + 1)).second;
        }
      }
      if (wanted[0]) {
        for (uint64_t k = 0; k < req.n; ++k) {
          const swg_closure_row& w = rows[k];
          std::string& o = text[0];
          o += swg_paf_sequence_name(p, w.seq);
          o += '\t';
          append_u64(o, w.start, '\t');
          append_u64(o, w.end, '\t');
          o += bed_text[w.region].label;
          o += '\t';
          append_u64(o, w.hop, '\n');
        }
      }
      if (wanted[1]) {
        for (uint64_t r = 0; r < m; ++r) {
          const swg_closure_summary& s = summary[r];
          std::string& o = text[1];
          o += bed_text[r].label;
          o += '\t';
          o += bed_text[r].name;
          o += '\t';
          append_u64(o, regions[r].start, '\t');
          append_u64(o, regions[r].end, '\t');
          append_u64(o, s.pieces, '\t');
          append_u64(o, s.sequences, '\t');
          append_u64(o, genomes[r], '\t');
          append_u64(o, s.bases, '\t');
          append_u64(o, s.hops, '\t');
          o += regions[r].seq == UINT32_MAX ? "unknown\n" : s.hops == 0 ? "none\n" : s.flags & SWG_CLOSURE_CUT ? "cut\n" : "closed\n";
        }
      }
    }
    return texts_hand_over(text, wanted, 2, out_text, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
