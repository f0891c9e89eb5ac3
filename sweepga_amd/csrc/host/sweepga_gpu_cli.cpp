// sweepga-gpu: the reference's filter-path command line (`sweepga <paf> --output-file out.paf ...`) with
// PafFilter::apply_filters running on an MI355X through libsweepga_gpu.so.
//
// Host side only, written in C++ because the reference's host is compiled code (Rust; no Rust toolchain in
// this image):
//   flags and defaults ........ src/cli.rs:204-288; flag -> FilterConfig mapping src/main.rs:3477-3568, 3590-3619
//   parse_filter_mode ......... src/main.rs:244-293        parse_metric_number / parse_identity_value ... src/cli.rs:26-130
//   extract_metadata .......... src/paf_filter.rs:292-376  parse_cigar_counts ... src/paf.rs:32-64
//   name interning ............ src/sequence_index.rs:7-31 genome prefixes ... src/paf_filter.rs:1022-1030,
//                                                          src/plane_sweep_scaffold.rs:13-22
//   write_filtered_output ..... src/paf_filter.rs:1689-1726
//   --joblist ................. src/main.rs:2711-2745 over FASTA input: one wfmash command per selected haplotype pair,
//                               sketches / distances / random pairs on the GPU (swg_joblist)
// Everything between "records parsed" and "per-record status + chain id" is one swg_filter() call.
// There is no CPU filter in this binary: without a GPU it exits with the library's error.
#include <unistd.h>

#include <cerrno>
#include <sys/mman.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "../../../include/sweepga_gpu.h"

namespace {

[[noreturn]] void die(int code, const std::string& msg) {
  std::fprintf(stderr, "sweepga-gpu: %s\n", msg.c_str());
  std::exit(code);
}

// ---- Rust-compatible scalar parsers -----------------------------------------------------------------
bool parse_u64(std::string_view s, uint64_t* out) {  // str::parse::<u64>
  size_t i = 0;
  if (s.empty()) return false;
  if (s[0] == '+') i = 1;
  if (i >= s.size()) return false;
  uint64_t v = 0;
  for (; i < s.size(); ++i) {
    const char c = s[i];
    if (c < '0' || c > '9') return false;
    const uint64_t d = (uint64_t)(c - '0');
    if (v > (UINT64_MAX - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = v;
  return true;
}
bool parse_f64(std::string_view sv, double* out) {  // str::parse::<f64>: no whitespace, no hex floats
  if (sv.empty()) return false;
  for (char c : sv)
    if (c == 'x' || c == 'X' || c == ' ' || c == '\t' || c == '\n' || c == '(') return false;
  std::string s(sv);
  char* e = nullptr;
  const double v = std::strtod(s.c_str(), &e);
  if (e == s.c_str() || *e != '\0') return false;
  *out = v;
  return true;
}
bool parse_int(const std::string& t, int* out) {  // decimal digits only
  if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos) return false;
  *out = std::atoi(t.c_str());
  return true;
}
bool parse_metric_number(const std::string& s, uint64_t* out) {  // cli.rs:26-61
  if (s.empty()) return false;
  std::string num = s;
  char suffix = 0;
  const char last = s.back();
  if ((last >= 'a' && last <= 'z') || (last >= 'A' && last <= 'Z')) {
    suffix = last;
    num = s.substr(0, s.size() - 1);
  }
  double base;
  if (!parse_f64(num, &base)) return false;
  double mult = 1.0;
  switch (suffix) {
    case 0: break;
    case 'k': case 'K': mult = 1e3; break;
    case 'm': case 'M': mult = 1e6; break;
    case 'g': case 'G': mult = 1e9; break;
    default: return false;
  }
  const double r = base * mult;
  if (r > (double)UINT64_MAX) return false;
  *out = !(r > 0.0) ? 0 : (r >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)r);
  return true;
}
int parse_scoring(const std::string& s) {  // main.rs:3485-3492
  if (s == "ani" || s == "identity") return SWG_SCORE_IDENTITY;
  if (s == "length") return SWG_SCORE_LENGTH;
  if (s == "length-ani" || s == "length-identity") return SWG_SCORE_LENGTH_IDENTITY;
  if (s == "matches") return SWG_SCORE_MATCHES;
  return SWG_SCORE_LOG_LENGTH_IDENTITY;
}
// main.rs:244-293.  Returns false for a bare "0" (the reference exits the process there).
bool parse_filter_mode(const std::string& mode, int32_t* fmode, uint64_t* pq, uint64_t* pt) {
  const std::string INF = "\xE2\x88\x9E";
  std::string lower = mode;
  for (auto& c : lower)
    if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
  auto set = [&](int m, uint64_t q, uint64_t t) {
    *fmode = m;
    *pq = q;
    *pt = t;
    return true;
  };
  if (lower == "1:1") return set(SWG_MODE_ONE_TO_ONE, 1, 1);
  if (lower == "1" || lower == "1:" + INF || lower == "1:infinity" || lower == "1:many") return set(SWG_MODE_ONE_TO_MANY, 1, 0);
  if (lower == INF + ":1" || lower == "infinity:1" || lower == "many:1") return set(SWG_MODE_MANY_TO_MANY, 0, 1);
  if (lower == "many:many" || lower == INF + ":" + INF || lower == "infinity:infinity" || lower == "many" || lower == INF ||
      lower == "infinity" || lower == "-1" || lower == "-1:-1")
    return set(SWG_MODE_MANY_TO_MANY, 0, 0);
  const size_t colon = lower.find(':');
  if (colon != std::string::npos) {
    if (lower.find(':', colon + 1) != std::string::npos) return set(SWG_MODE_ONE_TO_ONE, 1, 1);  // parts.len() != 2
    auto side = [&](const std::string& p) -> uint64_t {
      if (p == INF || p == "infinity" || p == "many" || p == "-1") return 0;
      uint64_t v;
      return parse_u64(p, &v) && v > 0 ? v : 0;
    };
    const uint64_t q = side(lower.substr(0, colon)), t = side(lower.substr(colon + 1));
    const int m = (q == 1 && t == 1) ? SWG_MODE_ONE_TO_ONE : (q == 1 && t == 0) ? SWG_MODE_ONE_TO_MANY : SWG_MODE_MANY_TO_MANY;
    return set(m, q, t);
  }
  uint64_t n;
  if (parse_u64(mode, &n)) {
    if (n == 0) return false;
    return set(SWG_MODE_ONE_TO_MANY, n, 0);
  }
  return set(SWG_MODE_ONE_TO_ONE, 1, 1);
}
// --sparsify (src/knn_graph.rs:59-160, src/main.rs:3494-3509).  `none`, `all`, a bare fraction and `random:<f>` have no
// effect on the PAF path (the filter never reads FilterConfig.sparsity).  `tree:` / `knn:` make the reference run
// tree_filter::apply_tree_filter_to_paf on the input BEFORE the filter (src/main.rs:3640-3688).  0 = fine (no effect),
// 1 = a strategy that is "not valid for post-alignment PAF/1aln filtering", 2 = unparsable, 3 = tree sampling (parameters
// returned through the pointers).
int check_sparsify(const std::string& v, unsigned long* tree_near = nullptr, unsigned long* tree_far = nullptr, double* tree_rand = nullptr) {
  auto frac_ok = [](const std::string& t, bool open_top) {
    char* e = nullptr;
    const double f = std::strtod(t.c_str(), &e);
    if (t.empty() || e == t.c_str() || *e) return false;
    return f > 0.0 && (open_top ? f < 1.0 : f <= 1.0);
  };
  {
    char* e = nullptr;
    const double f = std::strtod(v.c_str(), &e);
    if (!v.empty() && e != v.c_str() && !*e) return (f > 0.0 && f <= 1.0) ? 0 : 2;
  }
  if (v == "none" || v == "all") return 0;
  if (v == "auto") return 1;
  if (v.rfind("random:", 0) == 0) return frac_ok(v.substr(7), false) ? 0 : 2;
  if (v.rfind("giant:", 0) == 0 || v.rfind("connectivity:", 0) == 0) return frac_ok(v.substr(v.find(':') + 1), true) ? 1 : 2;
  if (v.rfind("wfmash:", 0) == 0) return (v.substr(7) == "auto" || frac_ok(v.substr(7), false)) ? 1 : 2;
  if (v.rfind("tree:", 0) == 0 || v.rfind("knn:", 0) == 0) {
    const std::string body = v.substr(v.find(':') + 1);
    unsigned long kn = 0, kf = 0;
    double rf = 0.0;
    int parts = 0;
    for (size_t s0 = 0; s0 <= body.size(); ++parts) {
      const size_t c = body.find(':', s0);
      const std::string tok = body.substr(s0, c == std::string::npos ? std::string::npos : c - s0);
      char* e = nullptr;
      if (parts < 2) {
        if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos) return 2;
        (parts == 0 ? kn : kf) = std::strtoul(tok.c_str(), &e, 10);
      } else if (parts == 2) {
        rf = std::strtod(tok.c_str(), &e);
        if (tok.empty() || e == tok.c_str() || *e) return 2;
      } else {
        return 2;
      }
      if (c == std::string::npos) {
        ++parts;
        break;
      }
      s0 = c + 1;
    }
    if (parts > 3 || (kn == 0 && kf == 0) || rf < 0.0 || rf > 1.0) return 2;
    if (tree_near) *tree_near = kn;
    if (tree_far) *tree_far = kf;
    if (tree_rand) *tree_rand = rf;
    return 3;
  }
  return 2;
}

// --joblist (src/main.rs:2711-2745): PanSN FASTA in, one `wfmash` command per selected haplotype pair out.  Every
// --sparsify value is valid here.  The GPU is opened when there is one; strategies that need it (sketches, random pairs)
// fail with the library's message without one.
int run_joblist(const std::vector<std::string>& inputs, const std::string& sparsify, uint64_t k, uint64_t s, uint64_t wfmash_threads,
                uint64_t min_aln_length, const std::string& dir, const std::string& output_file, int device) {
  if (inputs.empty()) die(1, "--joblist requires FASTA input");
  for (size_t i = 1; i <= dir.size(); ++i) {  // create_dir_all
    if (i < dir.size() && dir[i] != '/') continue;
    const std::string prefix = dir.substr(0, i);
    struct stat sb;
    if (stat(prefix.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode)) continue;
    if (mkdir(prefix.c_str(), 0777) != 0 && errno != EEXIST) die(1, "Failed to create joblist output dir '" + dir + "': " + std::strerror(errno));
  }
  swg_ctx* ctx = nullptr;
  if (swg_create(device, &ctx) != SWG_OK) ctx = nullptr;
  std::vector<const char*> paths;
  for (const auto& p : inputs) paths.push_back(p.c_str());
  char* text = nullptr;
  uint64_t len = 0;
  // out-of-range values stay out of range through the narrowing; the library refuses them only where a sketch is drawn
  const int kk = (int)std::min<uint64_t>(k, 1u << 30);
  const int rc = swg_joblist(ctx, paths.data(), (int)paths.size(), sparsify.c_str(), kk, s, wfmash_threads, min_aln_length, dir.c_str(), 0,
                             &text, &len, nullptr);
  if (rc != SWG_OK) die(1, swg_last_error(ctx));
  FILE* out = output_file.empty() ? stdout : std::fopen(output_file.c_str(), "wb");
  if (!out) die(1, "cannot open " + output_file + ": " + std::strerror(errno));
  if (len && std::fwrite(text, 1, len, out) != len) die(1, "write failed");
  if (out != stdout) std::fclose(out);
  swg_free(text);
  std::fflush(stdout);
  if (ctx) swg_destroy(ctx);
  return 0;
}

// One report file: "-" = standard error (flushed), an empty path = not asked for, nothing is written.
void write_bytes(const std::string& path, const char* data, uint64_t len) {
  if (path.empty()) return;
  FILE* f = path == "-" ? stderr : std::fopen(path.c_str(), "wb");
  if (!f) die(2, "cannot open " + path + ": " + std::strerror(errno));
  if (len && std::fwrite(data, 1, len, f) != len) die(2, "write to " + path + " failed");
  if (f != stderr && std::fclose(f) != 0) die(2, "write to " + path + " failed");
  if (f == stderr) std::fflush(stderr);
}
// ... of a text the library handed out, which is released
void write_text(const std::string& path, char* text, uint64_t len) {
  write_bytes(path, text, len);
  swg_free(text);
}
void write_texts(const std::string* const* paths, char* const* text, const uint64_t* len, int count) {
  for (int k = 0; k < count; ++k) write_text(*paths[k], text[k], len[k]);
}

// --stats: the bytes `alnstats <input> <output>` prints for the two files (compare_stats), with --stats-detailed followed by
// the two `alnstats <file> -d` reports (input, then output).  "-" = standard error: standard output may carry the PAF.
void write_stats_report(const std::string& path, const swg_alnstats* before, const swg_alnstats* after, const std::string& in_label,
                        const std::string& out_label, bool detailed) {
  std::string all;
  char* text = nullptr;
  uint64_t len = 0;
  if (swg_alnstats_compare(before, after, in_label.c_str(), out_label.c_str(), &text, &len) != SWG_OK)
    die(3, std::string("--stats: ") + swg_alnstats_last_error());
  all.assign(text, len);
  swg_free(text);
  if (detailed)
    for (int k = 0; k < 2; ++k) {
      if (swg_alnstats_report(k ? after : before, (k ? out_label : in_label).c_str(), 1, &text, &len) != SWG_OK)
        die(3, std::string("--stats-detailed: ") + swg_alnstats_last_error());
      all.append(text, len);
      swg_free(text);
    }
  write_bytes(path, all.data(), all.size());
}

// --breadth: the report of swg_paf_breadth (merged-interval coverage per genome pair, all records and the kept ones).
// "-" = standard error.
void write_breadth_report(const std::string& path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, bool detailed) {
  char* text = nullptr;
  uint64_t len = 0;
  if (swg_paf_breadth(ctx, paf, status, detailed ? 1 : 0, &text, &len) != SWG_OK) die(3, std::string("--breadth: ") + swg_alnstats_last_error());
  write_text(path, text, len);
}

// --blocks: the text of swg_paf_blocks (one PAF line per kept scaffold chain).  "-" = standard error.  status == NULL: no filter
// ran, there are no chains, the file is written empty.
void write_blocks(const std::string& path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, const uint32_t* chain) {
  char* text = nullptr;
  uint64_t len = 0;
  if (status && swg_paf_blocks(ctx, paf, status, chain, &text, &len) != SWG_OK) die(3, std::string("--blocks: ") + swg_alnstats_last_error());
  write_text(path, text, len);
}

// --components: the report of swg_paf_components (each sequence's component under the kept mappings).  "-" = standard error.
void write_components(const std::string& path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, const swg_component_params& par,
                      bool detailed) {
  char* text = nullptr;
  uint64_t len = 0;
  if (swg_paf_components(ctx, paf, status, &par, detailed ? 1 : 0, &text, &len) != SWG_OK)
    die(3, std::string("--components: ") + swg_alnstats_last_error());
  write_text(path, text, len);
}

// --lost / --covered: the LOST and KEPT texts of swg_paf_interval_texts (where coverage went, where it stayed), both from one
// device call when both are asked for.  "-" = standard error.
void write_intervals(const std::string& lost_path, const std::string& covered_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status) {
  char* text[3] = {nullptr, nullptr, nullptr};
  uint64_t len[3] = {0, 0, 0};
  const uint32_t sets = (lost_path.empty() ? 0u : 1u << SWG_IV_LOST) | (covered_path.empty() ? 0u : 1u << SWG_IV_KEPT);
  if (swg_paf_interval_texts(ctx, paf, status, sets, text, len) != SWG_OK) die(3, std::string("--lost / --covered: ") + swg_alnstats_last_error());
  write_text(lost_path, text[SWG_IV_LOST], len[SWG_IV_LOST]);
  write_text(covered_path, text[SWG_IV_KEPT], len[SWG_IV_KEPT]);
}

// --sharing / --sharing-bed: the table and the BED of swg_paf_sharing (how many genomes cover each base), both from one device call
// when both are asked for.  "-" = standard error.
void write_sharing(const std::string& table_path, const std::string& bed_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, bool detailed) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {table_path.empty() ? nullptr : &marker, bed_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  if (swg_paf_sharing(ctx, paf, status, detailed ? 1 : 0, text, len) != SWG_OK) die(3, std::string("--sharing: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&table_path, &bed_path};
  write_texts(paths, text, len, 2);
}

// --mosaic / --mosaic-share: the rows and the share table of swg_paf_mosaic (the best mapping at every base), both from one device
// call when both are asked for.  "-" = standard error.
void write_mosaic(const std::string& rows_path, const std::string& share_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, uint32_t axis,
                  uint32_t set, bool by_length) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {rows_path.empty() ? nullptr : &marker, share_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  if (swg_paf_mosaic(ctx, paf, status, axis, set, by_length ? 1 : 0, text, len) != SWG_OK) die(3, std::string("--mosaic: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&rows_path, &share_path};
  write_texts(paths, text, len, 2);
}

// --windows / --windows-summary: the rows and the summary of swg_paf_windows (depth, cover and identity per fixed window), both from
// one device call when both are asked for.  "-" = standard error.
void write_windows(const std::string& rows_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, uint32_t axis,
                   uint32_t window, const std::string& genome) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {rows_path.empty() ? nullptr : &marker, summary_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  if (swg_paf_windows(ctx, paf, status, axis, window, genome.empty() ? nullptr : genome.c_str(), text, len) != SWG_OK)
    die(3, std::string("--windows: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&rows_path, &summary_path};
  write_texts(paths, text, len, 2);
}

// --place / --place-summary: the rows and the summary of swg_paf_place (every sequence ordered and oriented along its best partner),
// both from one device call when both are asked for.  "-" = standard error.
void write_place(const std::string& rows_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, uint32_t axis,
                 uint32_t set, uint64_t min_bases) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {rows_path.empty() ? nullptr : &marker, summary_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  if (swg_paf_place(ctx, paf, status, axis, set, min_bases, text, len) != SWG_OK) die(3, std::string("--place: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&rows_path, &summary_path};
  write_texts(paths, text, len, 2);
}

// --gaps / --gaps-summary: the rows and the summary of swg_paf_gaps (the indel at every link of a kept chain, the captured
// inversions), both from one device call when both are asked for.  "-" = standard error.  status == NULL: no filter ran, there
// are no chains, the files hold their header lines.
void write_gaps(const std::string& rows_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status,
                const uint32_t* chain, uint32_t min_size) {
  char* text[2] = {nullptr, nullptr};
  uint64_t len[2] = {0, 0};
  const std::vector<uint8_t> none(swg_paf_records(paf)->n + 1, 0);  // (no filter: nothing takes part)
  const std::vector<uint32_t> zero(status ? 1 : none.size(), 0);
  if (swg_paf_gaps(ctx, paf, status ? status : none.data(), status ? chain : zero.data(), min_size, rows_path.empty() ? nullptr : &text[0],
                   rows_path.empty() ? nullptr : &len[0], summary_path.empty() ? nullptr : &text[1], summary_path.empty() ? nullptr : &len[1]) != SWG_OK)
    die(3, std::string("--gaps: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&rows_path, &summary_path};
  write_texts(paths, text, len, 2);
}

// --dotplot / --dotplot-layout: the image and the layout table of swg_paf_dotplot, both from one device call when both are asked
// for.  The layout's "-" = standard error.
void write_dotplot(const std::string& image_path, const std::string& layout_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status,
                   const swg_dot_view& view) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {image_path.empty() ? nullptr : &marker, layout_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  if (swg_paf_dotplot(ctx, paf, status, &view, text, len) != SWG_OK) die(3, std::string("--dotplot: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&image_path, &layout_path};
  write_texts(paths, text, len, 2);
}

// --lift / --lift-summary: the rows and the summary of swg_paf_lift (BED regions projected through the mappings), both from one
// device call when both are asked for.  "-" = standard error.  exact (--lift-exact): through swg_paf_lift_exact, the rows refined
// through the cg:Z: tags of the lines that are hit; what it met goes to standard error in one line.
void write_lift(const std::string& rows_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status,
                const std::string& bed, uint32_t set, uint32_t axes, bool exact, bool quiet) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {rows_path.empty() ? nullptr : &marker, summary_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  const int rc = exact ? swg_paf_lift_exact(ctx, paf, status, bed.data(), bed.size(), set, axes, text, len)
                       : swg_paf_lift(ctx, paf, status, bed.data(), bed.size(), set, axes, text, len);
  if (rc != SWG_OK) die(3, std::string(exact ? "--lift-exact: " : "--lift: ") + swg_alnstats_last_error());
  if (exact && !quiet) {
    uint64_t c[4];
    swg_paf_lift_exact_counts(c);
    std::fprintf(stderr, "[sweepga-gpu] --lift-exact: %llu records hit, %llu exact, %llu bad, %llu without a cg:Z: tag\n", (unsigned long long)c[0],
                 (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3]);
  }
  const std::string* paths[2] = {&rows_path, &summary_path};
  write_texts(paths, text, len, 2);
}

// --ucsc-chain: the liftOver chain file of swg_paf_ucsc_chain_write, one chain per record of the set from its cg:Z: CIGAR (blocks and
// their lines built on the device); what it met goes to standard error in one line.
void write_ucsc_chain(const std::string& path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, uint32_t set, uint32_t from, uint64_t batch,
                      bool quiet) {
  swg_ucsc_counts c;
  if (swg_paf_ucsc_chain_write(ctx, paf, status, set, from, path.c_str(), batch, &c) != SWG_OK) die(3, std::string("--ucsc-chain: ") + swg_alnstats_last_error());
  if (!quiet)
    std::fprintf(stderr, "[sweepga-gpu] --ucsc-chain: %llu chains of %llu records, %llu blocks, %llu bad, %llu beyond, %llu without a cg:Z: tag, "
                 "%llu without an aligned column\n", (unsigned long long)c.chains, (unsigned long long)c.records, (unsigned long long)c.blocks,
                 (unsigned long long)c.bad, (unsigned long long)c.beyond, (unsigned long long)c.untagged, (unsigned long long)c.empty);
}

// --lift-paf: the slices of swg_paf_lift_paf_write, one PAF line per lifted region and record with its own coordinates and the part of
// the record's cg:Z: CIGAR under the region (cut on the device); what it met goes to standard error in one line.
void write_lift_paf(const std::string& path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, const std::string& bed, uint32_t set, uint32_t axes,
                    uint32_t min_aligned, uint64_t batch, bool quiet) {
  swg_lift_paf_counts c;
  if (swg_paf_lift_paf_write(ctx, paf, status, bed.data(), bed.size(), set, axes, min_aligned, batch, path.c_str(), &c) != SWG_OK)
    die(3, std::string("--lift-paf: ") + swg_alnstats_last_error());
  if (!quiet)
    std::fprintf(stderr, "[sweepga-gpu] --lift-paf: %llu lines of %llu rows, %llu without a usable CIGAR, %llu without an aligned column, "
                 "%llu below --lift-paf-min-aligned, %llu bad CIGARs, %llu device calls\n", (unsigned long long)c.slices, (unsigned long long)c.rows,
                 (unsigned long long)c.interp, (unsigned long long)c.empty, (unsigned long long)c.too_short, (unsigned long long)c.bad,
                 (unsigned long long)c.batches);
}

// --diffs / --diffs-summary: the difference list of swg_paf_diffs_write, one row per X, I, D or N op of the set's cg:Z: CIGARs (built on
// the device), and its sums per genome pair; either path may be empty.  What it met goes to standard error in one line.
void write_diffs(const std::string& rows_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, uint32_t set,
                 uint32_t kinds, uint32_t min_indel, uint64_t batch, bool quiet) {
  swg_diff_counts c;
  if (swg_paf_diffs_write(ctx, paf, status, set, kinds, min_indel, batch, rows_path.empty() ? nullptr : rows_path.c_str(),
                          summary_path.empty() ? nullptr : summary_path.c_str(), &c) != SWG_OK)
    die(3, std::string("--diffs: ") + swg_alnstats_last_error());
  if (!quiet)
    std::fprintf(stderr, "[sweepga-gpu] --diffs: %llu rows of %llu usable entries in %llu records, %llu mismatched, %llu inserted, %llu deleted bases, "
                 "%llu columns under M ops, %llu bad, %llu without a cg:Z: tag\n", (unsigned long long)c.rows, (unsigned long long)c.usable,
                 (unsigned long long)c.records, (unsigned long long)c.snp_bases, (unsigned long long)c.ins_bases,
                 (unsigned long long)(c.del_bases + c.skip_bases), (unsigned long long)c.m_columns, (unsigned long long)c.bad, (unsigned long long)c.untagged);
}

// --vcf / --vcf-summary: the variant calls of swg_paf_vcf_write -- SNVs, insertions and deletions of the set's cg:Z: CIGARs with their
// bases from the FASTA records, as VCF 4.2 (built on the device) -- and their sums per genome pair; either path may be empty.  What it
// met goes to standard error in one line.  (The genome names were checked when the PAF was opened.)
void write_vcf(const std::string& vcf_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, const swg_fasta* fasta,
               uint32_t set, const std::string& ref, const std::string& query, uint32_t max_indel, uint64_t batch, bool quiet) {
  swg_vcf_options o{};
  o.set = set, o.max_indel = max_indel, o.batch_bytes = batch;
  o.ref_genome = ref.empty() ? nullptr : ref.c_str(), o.query_genome = query.empty() ? nullptr : query.c_str();
  swg_vcf_counts c;
  if (swg_paf_vcf_write(ctx, paf, status, fasta, &o, vcf_path.empty() ? nullptr : vcf_path.c_str(), summary_path.empty() ? nullptr : summary_path.c_str(),
                        &c) != SWG_OK)
    die(3, std::string("--vcf: ") + swg_alnstats_last_error());
  if (!quiet)
    std::fprintf(stderr, "[sweepga-gpu] --vcf: %llu variants (%llu SNVs, %llu insertions, %llu deletions), %llu same, %llu N columns, %llu equal under M ops, "
                 "%llu long, %llu unanchored, %llu entries without sequence, %llu out of sequence, %llu bad, %llu without a cg:Z: tag\n",
                 (unsigned long long)c.variants, (unsigned long long)c.snvs, (unsigned long long)c.n_ins,
                 (unsigned long long)c.n_del, (unsigned long long)c.same, (unsigned long long)c.n_columns, (unsigned long long)c.m_equal,
                 (unsigned long long)c.long_indels, (unsigned long long)c.unanchored, (unsigned long long)c.no_sequence, (unsigned long long)c.out_of_sequence,
                 (unsigned long long)c.bad, (unsigned long long)c.untagged);
}

// --maf: the MAF of swg_paf_maf_write -- the blocks of the set's records, the two rows of each gathered through the CIGAR on the device.
// What it met goes to standard error in one line.
void write_maf(const std::string& path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, const swg_fasta* fasta, uint32_t set, uint32_t split_gap,
               uint64_t batch, bool quiet) {
  swg_maf_options o{};
  o.set = set, o.split_gap = split_gap, o.batch_bytes = batch;
  swg_maf_counts c;
  if (swg_paf_maf_write(ctx, paf, status, fasta, &o, path.c_str(), &c) != SWG_OK) die(3, std::string("--maf: ") + swg_alnstats_last_error());
  if (quiet) return;
  std::fprintf(stderr, "[sweepga-gpu] --maf: %llu blocks of %llu records (%llu usable): %llu columns, %llu aligned; %llu breakers over %llu target and %llu "
               "query bases, %llu runs of gaps only; %llu entries without sequence, %llu out of sequence, %llu bad, %llu without a cg:Z: tag, %llu "
               "sequences of another length\n",
               (unsigned long long)c.blocks, (unsigned long long)c.records, (unsigned long long)c.usable, (unsigned long long)c.columns,
               (unsigned long long)c.aligned, (unsigned long long)c.breakers, (unsigned long long)c.skipped_t, (unsigned long long)c.skipped_q,
               (unsigned long long)c.gap_only, (unsigned long long)c.no_sequence, (unsigned long long)c.out_of_sequence, (unsigned long long)c.bad,
               (unsigned long long)c.untagged, (unsigned long long)c.length_mismatch);
}

// --eqx: the PAF of swg_paf_eqx_write -- the set's records with every cg:Z: resolved to =/X against the FASTA records, columns 10 and 11
// exact (built on the device).  What it met goes to standard error in one line; eq_wrong and x_wrong, when not zero, say that PAF and
// FASTA do not belong together.
void write_eqx(const std::string& path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, const swg_fasta* fasta, uint32_t set, uint32_t unresolved,
               uint64_t batch, bool quiet) {
  swg_eqx_options o{};
  o.set = set, o.unresolved = unresolved, o.batch_bytes = batch;
  swg_eqx_counts c;
  if (swg_paf_eqx_write(ctx, paf, status, fasta, &o, path.c_str(), &c) != SWG_OK) die(3, std::string("--eqx: ") + swg_alnstats_last_error());
  if (quiet) return;
  std::fprintf(stderr, "[sweepga-gpu] --eqx: %llu lines, %llu resolved (%llu changed): %llu columns, %llu matches, %llu mismatches, %llu under M ops; "
               "%llu entries without sequence, %llu out of sequence, %llu bad, %llu without a cg:Z: tag, %llu sequences of another length",
               (unsigned long long)c.lines, (unsigned long long)c.usable, (unsigned long long)c.changed, (unsigned long long)c.columns,
               (unsigned long long)c.matches, (unsigned long long)c.mismatches, (unsigned long long)c.m_columns, (unsigned long long)c.no_sequence,
               (unsigned long long)c.out_of_sequence, (unsigned long long)c.bad, (unsigned long long)c.untagged, (unsigned long long)c.length_mismatch);
  if (c.eq_wrong || c.x_wrong)
    std::fprintf(stderr, "; eq_wrong %llu, x_wrong %llu: '=' over differing and 'X' over equal bases -- is this the FASTA the PAF was made from?",
                 (unsigned long long)c.eq_wrong, (unsigned long long)c.x_wrong);
  std::fputc('\n', stderr);
}

// --divergence / --divergence-summary: the two texts of swg_paf_divergence (exact matches, mismatches and indels per fixed window,
// from the set's cg:Z: CIGARs, built on the device).  "-" = standard error.  What it met goes to standard error in one line.
void write_divergence(const std::string& rows_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status, uint32_t set,
                      uint32_t axis, uint32_t window, const std::string& genome, uint64_t batch, bool quiet) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {rows_path.empty() ? nullptr : &marker, summary_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  swg_divergence_counts c;
  if (swg_paf_divergence(ctx, paf, status, set, axis, window, genome.empty() ? nullptr : genome.c_str(), batch, text, len, &c) != SWG_OK)
    die(3, std::string("--divergence: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&rows_path, &summary_path};
  write_texts(paths, text, len, 2);
  if (!quiet)
    std::fprintf(stderr, "[sweepga-gpu] --divergence: %llu windows on %llu sequences from %llu usable entries of %llu records, %llu bad, "
                 "%llu without a cg:Z: tag\n", (unsigned long long)c.windows, (unsigned long long)c.seqs, (unsigned long long)c.usable,
                 (unsigned long long)c.records, (unsigned long long)c.bad, (unsigned long long)c.untagged);
}

// --lift-closure / --lift-closure-summary: the two texts of swg_paf_lift_closure (the regions walked through the mappings for up to
// `hops` hops), both from one walk.  "-" = standard error.
void write_lift_closure(const std::string& rows_path, const std::string& summary_path, swg_ctx* ctx, const swg_paf* paf, const uint8_t* status,
                        const std::string& bed, uint32_t set, uint32_t axes, uint32_t hops, uint32_t min_len) {
  char marker = 0;  // (a text is asked for by a non-NULL entry)
  char* text[2] = {rows_path.empty() ? nullptr : &marker, summary_path.empty() ? nullptr : &marker};
  uint64_t len[2] = {0, 0};
  if (swg_paf_lift_closure(ctx, paf, status, bed.data(), bed.size(), set, axes, hops, min_len, text, len) != SWG_OK)
    die(3, std::string("--lift-hops: ") + swg_alnstats_last_error());
  const std::string* paths[2] = {&rows_path, &summary_path};
  write_texts(paths, text, len, 2);
}

// --dotplot-size: N or WxH, each side in 1 .. 16384
bool parse_dot_size(const std::string& v, uint32_t* w, uint32_t* h) {
  auto side = [](const std::string& t, uint32_t* out) {
    if (t.empty() || t.size() > 5 || t.find_first_not_of("0123456789") != std::string::npos) return false;
    const int x = std::atoi(t.c_str());
    if (x < 1 || x > 16384) return false;
    *out = (uint32_t)x;
    return true;
  };
  const size_t x = v.find('x');
  if (x == std::string::npos) {
    if (!side(v, w)) return false;
    *h = *w;
    return true;
  }
  return side(v.substr(0, x), w) && side(v.substr(x + 1), h);
}

}  // namespace

int main(int argc, char** argv) {
  const auto t_main = std::chrono::steady_clock::now();
  std::string input, output_file;
  std::string num_mappings = "many:many", scoring = "log-length-ani", min_identity = "0";
  std::string scaffold_filter = "many:many", min_scaffold_identity = "0", ani_method_s = "n100";
  double overlap = 0.95, scaffold_overlap = 0.5;
  uint64_t scaffold_jump = 50000, scaffold_mass = 10000, scaffold_dist = 0, block_length = 0;
  bool keep_self = false, no_filter = false, scaffolds_only = false, quiet = false;
  int device = 0, threads = 0;
  std::vector<int> devices;
  std::string bad_sparsify, tree_sparsify, sparsify = "none", joblist_dir = ".";
  std::vector<std::string> inputs;
  bool joblist = false, threads_given = false, stats_detailed = false;
  std::string stats_path;  // --stats: empty = no report
  std::string breadth_path;  // --breadth: empty = no report
  bool breadth_detailed = false;
  std::string blocks_path;  // --blocks: empty = no file
  std::string gaps_path, gaps_summary_path;  // --gaps, --gaps-summary: empty = no file
  uint64_t gaps_min_size = 50;
  bool gaps_flag = false;  // (--gaps-min-size was given)
  std::string components_path;  // --components: empty = no report
  bool components_detailed = false, component_flag = false;  // (component_flag: one of the two threshold flags was given)
  swg_component_params component_par{0, 0, 0};
  std::string lost_path, covered_path;  // --lost, --covered: empty = no file
  std::string sharing_path, sharing_bed_path;  // --sharing, --sharing-bed: empty = no file
  bool sharing_detailed = false;
  std::string mosaic_path, mosaic_share_path;  // --mosaic, --mosaic-share: empty = no file
  uint32_t mosaic_axis = 0, mosaic_set = SWG_IV_KEPT;
  std::string place_path, place_summary_path;  // --place, --place-summary: empty = no file
  uint32_t place_axis = 0, place_set = SWG_IV_KEPT;
  uint64_t place_min_bases = 0;
  bool place_flag = false;  // (one of --place-axis / --place-set / --place-min-bases was given)
  std::string windows_path, windows_summary_path, windows_genome;  // --windows, --windows-summary: empty = no file; --windows-genome: empty = any
  uint32_t windows_axis = 0;
  uint64_t window_size = 10000;
  bool windows_flag = false;  // (one of --window-size / --windows-axis / --windows-genome was given)
  bool mosaic_by_length = false, mosaic_flag = false;  // (mosaic_flag: one of --mosaic-axis / --mosaic-set / --mosaic-by was given)
  std::string dotplot_path, dotplot_layout_path, dotplot_query, dotplot_target;  // --dotplot, --dotplot-layout: empty = no file
  swg_dot_view dot_view{2048, 2048, nullptr, nullptr};
  bool dotplot_flag = false;  // (one of --dotplot-size / --dotplot-query / --dotplot-target was given)
  std::string lift_regions_path, lift_path, lift_summary_path, lift_bed;  // --lift-regions, --lift, --lift-summary: empty = not given
  uint32_t lift_set = SWG_IV_KEPT, lift_axes = SWG_LIFT_AXIS_QUERY | SWG_LIFT_AXIS_TARGET;
  bool lift_flag = false;  // (--lift-set or --lift-axis was given)
  std::string lift_paf_path;  // --lift-paf: empty = no file
  uint64_t lift_paf_min_aligned = 1, lift_batch = 0;  // --lift-paf-min-aligned; --lift-batch: 0 = the library's default
  bool lift_paf_flag = false;  // (--lift-paf-min-aligned or --lift-batch was given)
  bool lift_exact = false;  // --lift-exact: the rows of --lift through the CIGARs
  std::string ucsc_path;    // --ucsc-chain: empty = no file
  uint32_t ucsc_from = SWG_UCSC_FROM_TARGET, ucsc_set = SWG_IV_KEPT;
  uint64_t ucsc_batch = 0;  // --ucsc-chain-batch: 0 = the library's default
  bool ucsc_flag = false;   // (one of --ucsc-chain-from / --ucsc-chain-set / --ucsc-chain-batch was given)
  std::string diffs_path, diffs_summary_path;  // --diffs, --diffs-summary: empty = not given
  uint32_t diffs_set = SWG_IV_KEPT, diffs_kinds = SWG_DIFF_SNP | SWG_DIFF_INS | SWG_DIFF_DEL;
  uint64_t diffs_min_indel = 1, diffs_batch = 0;  // --diffs-min-indel; --diffs-batch: 0 = the library's default
  bool diffs_flag = false;  // (one of --diffs-set / --diffs-kinds / --diffs-min-indel / --diffs-batch was given)
  std::string vcf_path, vcf_summary_path, vcf_ref, vcf_query;  // --vcf, --vcf-summary, --vcf-ref, --vcf-query: empty = not given
  std::vector<std::string> vcf_fasta_paths;                    // --vcf-fasta, once per file
  uint32_t vcf_set = SWG_IV_KEPT;
  uint64_t vcf_max_indel = 10000, vcf_batch = 0;  // --vcf-max-indel: 0 = no limit; --vcf-batch: 0 = the library's default
  bool vcf_flag = false;  // (a sub-option of --vcf was given)
  std::string eqx_path;                     // --eqx: empty = not given
  std::vector<std::string> eqx_fasta_paths;  // --eqx-fasta, once per file
  uint32_t eqx_set = SWG_IV_KEPT, eqx_unresolved = SWG_EQX_KEEP;
  uint64_t eqx_batch = 0;  // --eqx-batch: 0 = the library's default
  bool eqx_flag = false;   // (a sub-option of --eqx was given)
  std::string maf_path;                     // --maf: empty = not given
  std::vector<std::string> maf_fasta_paths;  // --maf-fasta, once per file
  uint32_t maf_set = SWG_IV_KEPT;
  uint64_t maf_split_gap = 0, maf_batch = 0;  // --maf-split-gap: 0 = one block per record; --maf-batch: 0 = the library's default
  bool maf_flag = false;                      // (a sub-option of --maf was given)
  std::string divergence_path, divergence_summary_path, divergence_genome;  // --divergence, --divergence-summary: empty = no file; -genome: empty = any
  uint32_t divergence_set = SWG_IV_KEPT, divergence_axis = 0;
  uint64_t divergence_window = 10000, divergence_batch = 0;  // --divergence-window; --divergence-batch: 0 = the library's default
  bool divergence_flag = false;  // (one of the --divergence-* sub-options was given)
  std::string closure_path, closure_summary_path;  // --lift-closure, --lift-closure-summary: empty = not given
  uint64_t lift_hops = 0, lift_min_length = 100;   // --lift-hops (0 = not given), --lift-min-length
  bool lift_min_length_flag = false;
  uint64_t mash_k = 15, mash_s = 1000;  // mash.rs:11-15
  unsigned long tree_near = 0, tree_far = 0;
  double tree_rand = 0.0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i], val;
    const size_t eq = a.find('=');
    const bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
    if (has_eq) {
      val = a.substr(eq + 1);
      a = a.substr(0, eq);
    }
    auto value = [&]() -> std::string {
      if (has_eq) return val;
      if (i + 1 >= argc) die(2, "missing value for " + a);
      return argv[++i];
    };
    if (a == "--output-file" || a == "-o") output_file = value();
    else if (a == "--num-mappings") num_mappings = value();
    else if (a == "--overlap") { if (!parse_f64(value(), &overlap)) die(2, "invalid value for --overlap"); }  // clap rejects it too
    else if (a == "--scoring") scoring = value();
    else if (a == "--min-aln-identity") min_identity = value();
    else if (a == "--min-aln-length") { if (!parse_metric_number(value(), &block_length)) die(2, "bad --min-aln-length"); }
    else if (a == "--self") keep_self = true;
    else if (a == "--no-filter") no_filter = true;
    else if (a == "--scaffold-jump") { if (!parse_metric_number(value(), &scaffold_jump)) die(2, "bad --scaffold-jump"); }
    else if (a == "--scaffold-mass") { if (!parse_metric_number(value(), &scaffold_mass)) die(2, "bad --scaffold-mass"); }
    else if (a == "--scaffold-filter") scaffold_filter = value();
    else if (a == "--scaffold-overlap") { if (!parse_f64(value(), &scaffold_overlap)) die(2, "invalid value for --scaffold-overlap"); }
    else if (a == "--scaffold-dist") { if (!parse_metric_number(value(), &scaffold_dist)) die(2, "bad --scaffold-dist"); }
    else if (a == "--min-scaffold-identity") min_scaffold_identity = value();
    else if (a == "--scaffolds-only") scaffolds_only = true;
    else if (a == "--ani-method") ani_method_s = value();
    else if (a == "--sparsify") {
      const std::string v = value();
      const int rc = check_sparsify(v, &tree_near, &tree_far, &tree_rand);
      if (rc == 2) die(2, "invalid value for --sparsify");
      if (rc == 1) bad_sparsify = v;  // reported after the --no-filter shortcut, as in main.rs:3461-3509
      tree_sparsify = rc == 3 ? v : std::string();
      sparsify = v;
    }
    else if (a == "--device") { if (!parse_int(value(), &device) || device < 0) die(2, "invalid value for --device"); }
    else if (a == "--devices") {  // comma-separated: shard the genome pairs over several GPUs of the node
      const std::string v = value();
      for (size_t s0 = 0; s0 <= v.size();) {
        const size_t c = v.find(',', s0);
        const std::string tok = v.substr(s0, c == std::string::npos ? std::string::npos : c - s0);
        if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos) die(2, "bad --devices");
        devices.push_back(std::atoi(tok.c_str()));
        if (c == std::string::npos) break;
        s0 = c + 1;
      }
    }
    else if (a == "--quiet") quiet = true;
    else if (a == "--no-adaptive-scaffolds" || a == "--paf") { /* no effect for PAF input (main.rs:3515-3527) */ }
    else if (a == "--threads" || a == "-t") {
      if (!parse_int(value(), &threads) || threads < 0) die(2, "invalid value for --threads");
      threads_given = true;
    }
    else if (a == "--stats") { stats_path = value(); if (stats_path.empty()) die(2, "empty value for --stats"); }
    else if (a == "--stats-detailed") stats_detailed = true;
    else if (a == "--breadth") { breadth_path = value(); if (breadth_path.empty()) die(2, "empty value for --breadth"); }
    else if (a == "--breadth-detailed") breadth_detailed = true;
    else if (a == "--blocks") { blocks_path = value(); if (blocks_path.empty()) die(2, "empty value for --blocks"); }
    else if (a == "--gaps") { gaps_path = value(); if (gaps_path.empty()) die(2, "empty value for --gaps"); }
    else if (a == "--gaps-summary") { gaps_summary_path = value(); if (gaps_summary_path.empty()) die(2, "empty value for --gaps-summary"); }
    else if (a == "--gaps-min-size") {
      if (!parse_metric_number(value(), &gaps_min_size) || gaps_min_size > 0xffffffffull) die(2, "bad --gaps-min-size");
      gaps_flag = true;
    }
    else if (a == "--components") { components_path = value(); if (components_path.empty()) die(2, "empty value for --components"); }
    else if (a == "--components-detailed") components_detailed = true;
    else if (a == "--lost") { lost_path = value(); if (lost_path.empty()) die(2, "empty value for --lost"); }
    else if (a == "--covered") { covered_path = value(); if (covered_path.empty()) die(2, "empty value for --covered"); }
    else if (a == "--sharing") { sharing_path = value(); if (sharing_path.empty()) die(2, "empty value for --sharing"); }
    else if (a == "--sharing-detailed") sharing_detailed = true;
    else if (a == "--sharing-bed") { sharing_bed_path = value(); if (sharing_bed_path.empty()) die(2, "empty value for --sharing-bed"); }
    else if (a == "--dotplot") {
      dotplot_path = value();
      if (dotplot_path.empty()) die(2, "empty value for --dotplot");
      if (dotplot_path == "-") die(2, "--dotplot writes a binary image: it needs a file");
    }
    else if (a == "--dotplot-layout") { dotplot_layout_path = value(); if (dotplot_layout_path.empty()) die(2, "empty value for --dotplot-layout"); }
    else if (a == "--dotplot-size") {
      const std::string v = value();
      if (v.empty()) die(2, "empty value for --dotplot-size");
      if (!parse_dot_size(v, &dot_view.width, &dot_view.height)) die(2, "invalid value for --dotplot-size: N or WxH, each side in 1 .. 16384");
      dotplot_flag = true;
    }
    else if (a == "--dotplot-query") { dotplot_query = value(); if (dotplot_query.empty()) die(2, "empty value for --dotplot-query"); dotplot_flag = true; }
    else if (a == "--dotplot-target") { dotplot_target = value(); if (dotplot_target.empty()) die(2, "empty value for --dotplot-target"); dotplot_flag = true; }
    else if (a == "--lift-regions") { lift_regions_path = value(); if (lift_regions_path.empty()) die(2, "empty value for --lift-regions"); }
    else if (a == "--lift") { lift_path = value(); if (lift_path.empty()) die(2, "empty value for --lift"); }
    else if (a == "--lift-summary") { lift_summary_path = value(); if (lift_summary_path.empty()) die(2, "empty value for --lift-summary"); }
    else if (a == "--lift-exact") lift_exact = true;
    else if (a == "--ucsc-chain") {
      ucsc_path = value();
      if (ucsc_path.empty()) die(2, "empty value for --ucsc-chain");
      if (ucsc_path == "-") die(2, "--ucsc-chain needs a file: a chain file is not a standard error report");
    }
    else if (a == "--ucsc-chain-from") {
      const std::string v = value();
      if (v == "target") ucsc_from = SWG_UCSC_FROM_TARGET;
      else if (v == "query") ucsc_from = SWG_UCSC_FROM_QUERY;
      else die(2, "invalid value for --ucsc-chain-from: target or query");
      ucsc_flag = true;
    }
    else if (a == "--ucsc-chain-set") {
      const std::string v = value();
      if (v == "kept") ucsc_set = SWG_IV_KEPT;
      else if (v == "all") ucsc_set = SWG_IV_ALL;
      else die(2, "invalid value for --ucsc-chain-set: kept or all");
      ucsc_flag = true;
    }
    else if (a == "--ucsc-chain-batch") {
      if (!parse_metric_number(value(), &ucsc_batch) || ucsc_batch == 0) die(2, "invalid value for --ucsc-chain-batch: 1 or more bytes");
      ucsc_flag = true;
    }
    else if (a == "--diffs" || a == "--diffs-summary") {
      std::string& path = a == "--diffs" ? diffs_path : diffs_summary_path;
      path = value();
      if (path.empty()) die(2, "empty value for " + a);
      if (path == "-") die(2, a + " needs a file: the difference list is not a standard error report");
    }
    else if (a == "--vcf" || a == "--vcf-summary") {
      std::string& path = a == "--vcf" ? vcf_path : vcf_summary_path;
      path = value();
      if (path.empty()) die(2, "empty value for " + a);
      if (path == "-") die(2, a + " needs a file: the variant calls are not a standard error report");
    }
    else if (a == "--vcf-fasta") {
      vcf_fasta_paths.push_back(value());
      if (vcf_fasta_paths.back().empty() || vcf_fasta_paths.back() == "-") die(2, "--vcf-fasta needs a file");
      vcf_flag = true;
    }
    else if (a == "--vcf-ref" || a == "--vcf-query") {
      std::string& name = a == "--vcf-ref" ? vcf_ref : vcf_query;
      name = value();
      if (name.empty()) die(2, "empty value for " + a);
      vcf_flag = true;
    }
    else if (a == "--vcf-set") {
      const std::string v = value();
      if (v == "kept") vcf_set = SWG_IV_KEPT;
      else if (v == "all") vcf_set = SWG_IV_ALL;
      else die(2, "invalid value for --vcf-set: kept or all");
      vcf_flag = true;
    }
    else if (a == "--vcf-max-indel") {
      if (!parse_metric_number(value(), &vcf_max_indel) || vcf_max_indel > 0xffffffffull) die(2, "invalid value for --vcf-max-indel: 0 .. 2^32 - 1");
      vcf_flag = true;
    }
    else if (a == "--vcf-batch") {
      if (!parse_metric_number(value(), &vcf_batch) || vcf_batch == 0) die(2, "invalid value for --vcf-batch: 1 or more bytes");
      vcf_flag = true;
    }
    else if (a == "--maf") {
      maf_path = value();
      if (maf_path.empty()) die(2, "empty value for --maf");
      if (maf_path == "-") die(2, "--maf needs a file: the MAF is not a standard error report");
    }
    else if (a == "--maf-fasta") {
      maf_fasta_paths.push_back(value());
      if (maf_fasta_paths.back().empty() || maf_fasta_paths.back() == "-") die(2, "--maf-fasta needs a file");
      maf_flag = true;
    }
    else if (a == "--maf-set") {
      const std::string v = value();
      if (v == "kept") maf_set = SWG_IV_KEPT;
      else if (v == "all") maf_set = SWG_IV_ALL;
      else die(2, "invalid value for --maf-set: kept or all");
      maf_flag = true;
    }
    else if (a == "--maf-split-gap") {
      if (!parse_metric_number(value(), &maf_split_gap) || maf_split_gap >> 32) die(2, "invalid value for --maf-split-gap: 0 .. 4294967295 bases");
      maf_flag = true;
    }
    else if (a == "--maf-batch") {
      if (!parse_metric_number(value(), &maf_batch) || maf_batch == 0) die(2, "invalid value for --maf-batch: 1 or more bytes");
      maf_flag = true;
    }
    else if (a == "--eqx") {
      eqx_path = value();
      if (eqx_path.empty()) die(2, "empty value for --eqx");
      if (eqx_path == "-") die(2, "--eqx needs a file: the resolved PAF is not a standard error report");
    }
    else if (a == "--eqx-fasta") {
      eqx_fasta_paths.push_back(value());
      if (eqx_fasta_paths.back().empty() || eqx_fasta_paths.back() == "-") die(2, "--eqx-fasta needs a file");
      eqx_flag = true;
    }
    else if (a == "--eqx-set") {
      const std::string v = value();
      if (v == "kept") eqx_set = SWG_IV_KEPT;
      else if (v == "all") eqx_set = SWG_IV_ALL;
      else die(2, "invalid value for --eqx-set: kept or all");
      eqx_flag = true;
    }
    else if (a == "--eqx-unresolved") {
      const std::string v = value();
      if (v == "keep") eqx_unresolved = SWG_EQX_KEEP;
      else if (v == "drop") eqx_unresolved = SWG_EQX_DROP;
      else die(2, "invalid value for --eqx-unresolved: keep or drop");
      eqx_flag = true;
    }
    else if (a == "--eqx-batch") {
      if (!parse_metric_number(value(), &eqx_batch) || eqx_batch == 0) die(2, "invalid value for --eqx-batch: 1 or more bytes");
      eqx_flag = true;
    }
    else if (a == "--diffs-set") {
      const std::string v = value();
      if (v == "kept") diffs_set = SWG_IV_KEPT;
      else if (v == "all") diffs_set = SWG_IV_ALL;
      else die(2, "invalid value for --diffs-set: kept or all");
      diffs_flag = true;
    }
    else if (a == "--diffs-kinds") {
      const std::string v = value() + ",";
      diffs_kinds = 0;
      for (size_t from = 0, to; (to = v.find(',', from)) != std::string::npos; from = to + 1) {
        const std::string w = v.substr(from, to - from);
        if (w == "snp") diffs_kinds |= SWG_DIFF_SNP;
        else if (w == "ins") diffs_kinds |= SWG_DIFF_INS;
        else if (w == "del") diffs_kinds |= SWG_DIFF_DEL;
        else if (w == "skip") diffs_kinds |= SWG_DIFF_SKIP;
        else if (!w.empty()) die(2, "invalid value for --diffs-kinds: a comma-separated list of snp, ins, del, skip");
      }
      if (!diffs_kinds) die(2, "invalid value for --diffs-kinds: the list is empty");
      diffs_flag = true;
    }
    else if (a == "--diffs-min-indel") {
      if (!parse_metric_number(value(), &diffs_min_indel) || diffs_min_indel > 0xffffffffull) die(2, "invalid value for --diffs-min-indel: 0 .. 2^32 - 1");
      diffs_flag = true;
    }
    else if (a == "--diffs-batch") {
      if (!parse_metric_number(value(), &diffs_batch) || diffs_batch == 0) die(2, "invalid value for --diffs-batch: 1 or more bytes");
      diffs_flag = true;
    }
    else if (a == "--divergence" || a == "--divergence-summary") {
      std::string& path = a == "--divergence" ? divergence_path : divergence_summary_path;
      path = value();
      if (path.empty()) die(2, "empty value for " + a);
    }
    else if (a == "--divergence-window") {
      if (!parse_metric_number(value(), &divergence_window) || divergence_window == 0 || divergence_window > 0xffffffffull)
        die(2, "invalid value for --divergence-window: 1 .. 2^32 - 1");
      divergence_flag = true;
    }
    else if (a == "--divergence-axis") {
      const std::string v = value();
      if (v == "query") divergence_axis = 0;
      else if (v == "target") divergence_axis = 1;
      else die(2, "invalid value for --divergence-axis: query or target");
      divergence_flag = true;
    }
    else if (a == "--divergence-genome") {
      divergence_genome = value();
      if (divergence_genome.empty()) die(2, "empty value for --divergence-genome");
      divergence_flag = true;
    }
    else if (a == "--divergence-set") {
      const std::string v = value();
      if (v == "kept") divergence_set = SWG_IV_KEPT;
      else if (v == "all") divergence_set = SWG_IV_ALL;
      else die(2, "invalid value for --divergence-set: kept or all");
      divergence_flag = true;
    }
    else if (a == "--divergence-batch") {
      if (!parse_metric_number(value(), &divergence_batch) || divergence_batch == 0) die(2, "invalid value for --divergence-batch: 1 or more bytes");
      divergence_flag = true;
    }
    else if (a == "--lift-hops") { if (!parse_u64(value(), &lift_hops) || lift_hops < 1 || lift_hops > 65535) die(2, "invalid value for --lift-hops: 1 .. 65535"); }
    else if (a == "--lift-closure") { closure_path = value(); if (closure_path.empty()) die(2, "empty value for --lift-closure"); }
    else if (a == "--lift-closure-summary") { closure_summary_path = value(); if (closure_summary_path.empty()) die(2, "empty value for --lift-closure-summary"); }
    else if (a == "--lift-min-length") {
      if (!parse_u64(value(), &lift_min_length) || lift_min_length > UINT32_MAX) die(2, "invalid value for --lift-min-length: 0 .. 2^32 - 1");
      lift_min_length_flag = true;
    }
    else if (a == "--place") { place_path = value(); if (place_path.empty()) die(2, "empty value for --place"); }
    else if (a == "--place-summary") { place_summary_path = value(); if (place_summary_path.empty()) die(2, "empty value for --place-summary"); }
    else if (a == "--place-axis") {
      const std::string v = value();
      if (v == "query") place_axis = 0;
      else if (v == "target") place_axis = 1;
      else die(2, "invalid value for --place-axis: query or target");
      place_flag = true;
    }
    else if (a == "--place-set") {
      const std::string v = value();
      if (v == "kept") place_set = SWG_IV_KEPT;
      else if (v == "all") place_set = SWG_IV_ALL;
      else die(2, "invalid value for --place-set: kept or all");
      place_flag = true;
    }
    else if (a == "--place-min-bases") {
      if (!parse_metric_number(value(), &place_min_bases)) die(2, "bad --place-min-bases");
      place_flag = true;
    }
    else if (a == "--windows") { windows_path = value(); if (windows_path.empty()) die(2, "empty value for --windows"); }
    else if (a == "--windows-summary") { windows_summary_path = value(); if (windows_summary_path.empty()) die(2, "empty value for --windows-summary"); }
    else if (a == "--window-size") {
      if (!parse_metric_number(value(), &window_size) || window_size == 0 || window_size > 0xffffffffull) die(2, "invalid value for --window-size: 1 .. 2^32 - 1");
      windows_flag = true;
    }
    else if (a == "--windows-axis") {
      const std::string v = value();
      if (v == "query") windows_axis = 0;
      else if (v == "target") windows_axis = 1;
      else die(2, "invalid value for --windows-axis: query or target");
      windows_flag = true;
    }
    else if (a == "--windows-genome") {
      windows_genome = value();
      if (windows_genome.empty()) die(2, "empty value for --windows-genome");
      windows_flag = true;
    }
    else if (a == "--mosaic") { mosaic_path = value(); if (mosaic_path.empty()) die(2, "empty value for --mosaic"); }
    else if (a == "--mosaic-share") { mosaic_share_path = value(); if (mosaic_share_path.empty()) die(2, "empty value for --mosaic-share"); }
    else if (a == "--mosaic-axis") {
      const std::string v = value();
      if (v == "query") mosaic_axis = 0;
      else if (v == "target") mosaic_axis = 1;
      else die(2, "invalid value for --mosaic-axis: query or target");
      mosaic_flag = true;
    }
    else if (a == "--mosaic-set") {
      const std::string v = value();
      if (v == "kept") mosaic_set = SWG_IV_KEPT;
      else if (v == "all") mosaic_set = SWG_IV_ALL;
      else die(2, "invalid value for --mosaic-set: kept or all");
      mosaic_flag = true;
    }
    else if (a == "--mosaic-by") {
      const std::string v = value();
      if (v == "matches") mosaic_by_length = false;
      else if (v == "length") mosaic_by_length = true;
      else die(2, "invalid value for --mosaic-by: matches or length");
      mosaic_flag = true;
    }
    else if (a == "--lift-paf") {
      lift_paf_path = value();
      if (lift_paf_path.empty()) die(2, "empty value for --lift-paf");
      if (lift_paf_path == "-") die(2, "--lift-paf needs a file: a PAF is not a standard error report");
    }
    else if (a == "--lift-paf-min-aligned") {
      if (!parse_metric_number(value(), &lift_paf_min_aligned) || lift_paf_min_aligned == 0 || lift_paf_min_aligned >> 32)
        die(2, "invalid value for --lift-paf-min-aligned: 1 .. 4294967295 aligned columns");
      lift_paf_flag = true;
    }
    else if (a == "--lift-batch") {
      if (!parse_metric_number(value(), &lift_batch) || lift_batch == 0) die(2, "invalid value for --lift-batch: 1 or more bytes");
      lift_paf_flag = true;
    }
    else if (a == "--lift-set") {
      const std::string v = value();
      if (v == "kept") lift_set = SWG_IV_KEPT;
      else if (v == "all") lift_set = SWG_IV_ALL;
      else die(2, "invalid value for --lift-set: kept or all");
      lift_flag = true;
    }
    else if (a == "--lift-axis") {
      const std::string v = value();
      if (v == "query") lift_axes = SWG_LIFT_AXIS_QUERY;
      else if (v == "target") lift_axes = SWG_LIFT_AXIS_TARGET;
      else if (v == "both") lift_axes = SWG_LIFT_AXIS_QUERY | SWG_LIFT_AXIS_TARGET;
      else die(2, "invalid value for --lift-axis: query, target or both");
      lift_flag = true;
    }
    else if (a == "--component-min-bases") {
      if (!parse_metric_number(value(), &component_par.min_bases)) die(2, "bad --component-min-bases");
      component_flag = true;
    }
    else if (a == "--component-min-share") {
      double share = 0.0;
      if (!parse_f64(value(), &share) || !(share >= 0.0 && share <= 1.0)) die(2, "invalid value for --component-min-share: a share in [0, 1]");
      component_par.min_share_ppm = (uint32_t)std::llround(share * 1e6);
      component_flag = true;
    }
    else if (a == "--joblist") joblist = true;
    else if (a == "--joblist-output-dir") joblist_dir = value();
    else if (a == "--mash-kmer-size") { if (!parse_u64(value(), &mash_k)) die(2, "invalid value for --mash-kmer-size"); }
    else if (a == "--mash-sketch-size") { if (!parse_u64(value(), &mash_s)) die(2, "invalid value for --mash-sketch-size"); }
    else if (a == "--help" || a == "-h") {
      std::puts("usage: sweepga-gpu <in.paf> [--output-file out.paf] [--num-mappings M] [--overlap F] [--scoring S]\n"
                "         [--min-aln-identity I] [--min-aln-length N] [--self] [--no-filter] [--scaffold-jump N]\n"
                "         [--scaffold-mass N] [--scaffold-filter M] [--scaffold-overlap F] [--scaffold-dist N]\n"
                "         [--min-scaffold-identity I] [--scaffolds-only] [--ani-method M]\n"
                "         [--device D | --devices D0,D1,...] [--threads T] [--quiet]\n"
                "         [--stats REPORT|-] [--stats-detailed] [--breadth REPORT|-] [--breadth-detailed]\n"
                "         [--blocks FILE|-]\n"
                "         [--gaps FILE|-] [--gaps-summary FILE|-] [--gaps-min-size N]\n"
                "         [--place FILE|-] [--place-summary FILE|-] [--place-axis query|target] [--place-set kept|all] [--place-min-bases N]\n"
                "         [--windows FILE|-] [--windows-summary FILE|-] [--window-size N] [--windows-axis query|target] [--windows-genome NAME]\n"
                "         [--components REPORT|-] [--components-detailed] [--component-min-bases N] [--component-min-share F]\n"
                "         [--lost FILE|-] [--covered FILE|-]\n"
                "         [--sharing REPORT|-] [--sharing-detailed] [--sharing-bed FILE|-]\n"
                "         [--mosaic FILE|-] [--mosaic-share FILE|-] [--mosaic-axis query|target] [--mosaic-set kept|all] [--mosaic-by matches|length]\n"
                "         [--dotplot FILE] [--dotplot-size N|WxH] [--dotplot-layout FILE|-] [--dotplot-query PREFIX] [--dotplot-target PREFIX]\n"
                "         [--lift-regions BED] [--lift FILE|-] [--lift-summary FILE|-] [--lift-set kept|all] [--lift-axis query|target|both]\n"
                "         [--lift-exact]\n"
                "         [--lift-paf FILE] [--lift-paf-min-aligned N] [--lift-batch BYTES]\n"
                "         [--ucsc-chain FILE] [--ucsc-chain-from target|query] [--ucsc-chain-set kept|all] [--ucsc-chain-batch BYTES]\n"
                "         [--diffs FILE] [--diffs-summary FILE] [--diffs-set kept|all] [--diffs-kinds snp,ins,del,skip] [--diffs-min-indel N]\n"
                "         [--diffs-batch BYTES]\n"
                "         [--vcf FILE] [--vcf-summary FILE] --vcf-fasta FASTA [--vcf-fasta FASTA ...] [--vcf-ref GENOME] [--vcf-query GENOME]\n"
                "         [--vcf-set kept|all] [--vcf-max-indel N] [--vcf-batch BYTES]\n"
                "         [--eqx FILE] --eqx-fasta FASTA [--eqx-fasta FASTA ...] [--eqx-set kept|all] [--eqx-unresolved keep|drop] [--eqx-batch BYTES]\n"
                "         [--maf FILE] --maf-fasta FASTA [--maf-fasta FASTA ...] [--maf-set kept|all] [--maf-split-gap N] [--maf-batch BYTES]\n"
                "         [--divergence FILE|-] [--divergence-summary FILE|-] [--divergence-window N] [--divergence-axis query|target]\n"
                "         [--divergence-genome NAME] [--divergence-set kept|all] [--divergence-batch BYTES]\n"
                "         [--lift-hops N] [--lift-closure FILE|-] [--lift-closure-summary FILE|-] [--lift-min-length N]\n"
                "       sweepga-gpu --joblist <in.fa[.gz]>... [--sparsify S] [--mash-kmer-size K] [--mash-sketch-size N]\n"
                "         [--joblist-output-dir DIR] [--threads T] [--min-aln-length L] [--output-file jobs.txt]\n"
                "  --stats REPORT      after the filter, before the output is written: what `alnstats <in.paf> <out.paf>` would print,\n"
                "                      computed on the device from the records and their status (- = standard error)\n"
                "  --stats-detailed    with --stats: followed by the two `alnstats <file> -d` reports (input, then output)\n"
                "  --breadth REPORT    after the filter: per set (all records, kept records) the bases of either side under at least one\n"
                "                      inter-genome mapping (merged intervals), their share of the genome and the mean depth, as a\n"
                "                      tab-separated table computed on the device (- = standard error); with --no-filter kept = all\n"
                "  --breadth-detailed  with --breadth: one row per ordered genome pair ahead of each set's `*` row of sums\n"
                "  --blocks FILE       after the filter: one PAF line per scaffold chain that was kept -- its span on both sequences, summed\n"
                "                      matches and block length, and the tags ch:Z: nc:i: ni:i: nr:i: (core, inverted, rescued mappings)\n"
                "                      qc:i: tc:i: (bases under at least one of them) id:f: -- built on the device (- = standard error);\n"
                "                      empty with --no-filter or --scaffold-jump 0, which make no chains\n"
                "  --gaps FILE         after the filter: what lies between the mappings of each kept chain -- one line per link whose\n"
                "                      unaligned query and target stretches differ by at least --gaps-min-size (INS / DEL; dq, dt negative\n"
                "                      = overlap) and per captured inversion (INV), `#query q_start q_end target t_start t_end kind size\n"
                "                      chain dq dt left right`, ordered by chain and query position -- built on the device (- = standard\n"
                "                      error); header only with --no-filter or --scaffold-jump 0, which make no chains\n"
                "  --gaps-summary FILE per genome pair `links ins ins_bases del del_bases inv inv_bases`, then the size spectrum as\n"
                "                      `#spectrum KIND lo hi count`; with --gaps, both come from one device call\n"
                "  --gaps-min-size N   the smallest |size| (INV: query length) that gives a line; k/m/g suffixes (default 50)\n"
                "  --place FILE        after the filter: every sequence ordered and oriented along its best partner of each other genome --\n"
                "                      `sequence length partner partner_length orient start end rank bases fwd rev total runner records\n"
                "                      q_lo q_hi t_lo t_hi`, in layout order (genome, partner genome, partner, start); start is the weighted\n"
                "                      median of where the mappings put base 0 of the sequence (signed); '-' = standard error\n"
                "  --place-summary FILE per genome pair `sequences reversed length bases total_bases`; with --place, both come from one\n"
                "                      device call\n"
                "  --place-axis query|target  the sequences that are placed (default query)\n"
                "  --place-set kept|all  the mappings that vote (default kept; with --no-filter kept = all)\n"
                "  --place-min-bases N a row needs a best partner with at least N aligned bases; k/m/g suffixes (default 0)\n"
                "  --windows FILE      after the filter: one line per window of every sequence that carries an inter-genome mapping --\n"
                "                      `sequence start end n_all depth_all covered_all matches_all n_kept depth_kept covered_kept matches_kept`\n"
                "                      (a BED / bedGraph source; integers: mean depth = depth / (end - start), identity = matches / depth,\n"
                "                      breadth = covered / (end - start)), before (all) and after (kept) the filter; '-' = standard error\n"
                "  --windows-summary FILE per sequence `length windows empty covered depth matches records`, all and kept side by side; with\n"
                "                      --windows, both come from one device call\n"
                "  --window-size N     the window in bases, 1 .. 2^32 - 1; k/m/g suffixes (default 10k)\n"
                "  --windows-axis query|target  the sequences the windows lie on (default query)\n"
                "  --windows-genome NAME  only the mappings whose other side belongs to this genome (default: any other genome)\n"
                "  --components REPORT after the filter: per sequence its component -- the connected sets of sequences over the links\n"
                "                      between sequence pairs that the kept mappings make -- with the component's sequences and length\n"
                "                      and the sequence's own links, records and bases, as a tab-separated table computed on the device\n"
                "                      (- = standard error); with --no-filter every record takes part\n"
                "  --components-detailed  with --components: one row per link (a b records a_bases b_bases joined) after `#links`\n"
                "  --component-min-bases N  with --components: a link joins only if the bases on one of its ends reach N (k/m/g)\n"
                "  --component-min-share F  with --components: ... and cover the share F in [0, 1] of one end's length\n"
                "  --lost FILE         after the filter: the stretches that lay under at least one inter-genome mapping before the filter\n"
                "                      and under none after it, as merged intervals per sequence and genome of the other side, one line\n"
                "                      `sequence start end other_genome q|t` each, built on the device (- = standard error); empty with\n"
                "                      --no-filter\n"
                "  --covered FILE      after the filter: the same lines for the stretches the kept mappings still cover (with --no-filter:\n"
                "                      those of all mappings); with --lost, both come from one device call\n"
                "  --sharing REPORT    after the filter: per genome the bases that no other genome covers (private), that every other\n"
                "                      genome covers (core) and the rest (shared), over all records and over the kept ones, as a\n"
                "                      tab-separated table; a genome covers a base when an inter-genome mapping to it lies over the base,\n"
                "                      from either side.  Built on the device (- = standard error); with --no-filter kept = all\n"
                "  --sharing-detailed  with --sharing: after `#spectrum`, `genome all|kept depth bases` for every depth that occurs\n"
                "  --sharing-bed FILE  after the filter: `sequence start end n_all n_kept`, the stretches covered by a constant number\n"
                "                      of genomes before (n_all >= 1) and after the filter; with --sharing, both come from one device call\n"
                "  --mosaic FILE       after the filter: the best mapping at every base -- `sequence start end other_sequence strand record\n"
                "                      weight other_start other_end`, one line per maximal stretch on which one inter-genome mapping is the\n"
                "                      heaviest (ties: the earlier record); a tiling of what is covered, built on the device (- = standard\n"
                "                      error), and a --lift-regions input\n"
                "  --mosaic-share FILE `genome other_genome bases`: how much of each genome every other genome wins, then `#total bases`;\n"
                "                      with --mosaic, both come from one device call\n"
                "  --mosaic-axis query|target  the sequences that are tiled (default query)\n"
                "  --mosaic-set kept|all  the mappings that compete (default kept; with --no-filter kept = all)\n"
                "  --mosaic-by matches|length  a mapping's weight: its matches column or its length on the axis (default matches)\n"
                "  --dotplot FILE      after the filter: a dot plot of the mappings as a binary PPM, targets along x and queries along y,\n"
                "                      sequences in (genome, first appearance) order, the origin bottom-left: kept mappings black, kept\n"
                "                      inversions red, dropped mappings grey, dropped inversions pink, genome borders pale blue.  Rasterised\n"
                "                      on the device; with --no-filter kept = all\n"
                "  --dotplot-size N|WxH  the image's size in pixels, each side in 1 .. 16384 (default 2048)\n"
                "  --dotplot-layout FILE  `axis sequence genome offset length first_pixel last_pixel` for every sequence of either axis\n"
                "                      (- = standard error); with --dotplot, both come from one device call\n"
                "  --dotplot-query PREFIX   only query sequences whose name starts with PREFIX go on the y axis\n"
                "  --dotplot-target PREFIX  only target sequences whose name starts with PREFIX go on the x axis\n"
                "  --lift-regions BED  regions (name start end [label]) to project through the mappings after the filter\n"
                "  --lift FILE         `dst_name dst_start dst_end label src_name src_start src_end strand axis record`: where each region\n"
                "                      lands on the other side of every mapping that covers it (linear interpolation, rounded outward;\n"
                "                      - = standard error)\n"
                "  --lift-summary FILE `label sequence start end all_q all_t kept_q kept_t state` per region: its hits before and after the\n"
                "                      filter; state lost = the filter left it without a projection; with --lift, one device call\n"
                "  --lift-exact        project the rows of --lift base by base through the cg:Z: CIGARs of the lines that are hit (parsed on\n"
                "                      the device): three more columns `aligned matches mode`, mode exact | interp (no usable CIGAR on the\n"
                "                      line: the interpolated row); needs --lift-regions and --lift; one line of counts on standard error\n"
                "  --ucsc-chain FILE   write a UCSC chain file (liftOver, CrossMap, bcftools +liftover): one chain per record from its cg:Z:\n"
                "                      CIGAR, blocks and block lines built on the device; one line of counts on standard error\n"
                "  --ucsc-chain-from target|query  which side is the chain's reference sequence (default target, as liftOver expects)\n"
                "  --ucsc-chain-set kept|all       the records that give chains (default kept)\n"
                "  --ucsc-chain-batch BYTES        CIGAR text per device call; k/m/g suffixes (default: from the device's memory; for tests)\n"
                "  --diffs FILE        write every mismatch run, insertion and deletion of the cg:Z: CIGARs, one line per X, I, D or N op (built on\n"
                "                      the device; adjacent ops are not merged): t_name t_start t_end q_name q_start q_end strand kind len left\n"
                "                      right record, left / right the '=' runs beside it; one line of counts on standard error\n"
                "  --diffs-summary FILE  per genome pair the aligned, matching, mismatched, inserted and deleted bases over all ops, and a length\n"
                "                      spectrum per kind; alone: the rows are counted and not built\n"
                "  --diffs-set kept|all            the records that are read (default kept)\n"
                "  --diffs-kinds LIST              the kinds that give rows: snp,ins,del,skip (default snp,ins,del)\n"
                "  --diffs-min-indel N             rows of ins, del and skip from N bases on (default 1; mismatches are never dropped)\n"
                "  --diffs-batch BYTES             CIGAR text per device call; k/m/g suffixes (default: from the device's memory; for tests)\n"
                "  --vcf FILE          write the variant calls of the cg:Z: CIGARs as VCF 4.2: one line per differing base under an X or M op and\n"
                "                      per insertion or deletion, with its bases from the FASTA records (built on the device); sorted per contig\n"
                "  --vcf-summary FILE  per genome pair the compared columns, the 12 substitution counts, insertions, deletions, ts and tv\n"
                "  --vcf-fasta FASTA               the sequences, matched to the PAF's names by exact name; once per file (needed)\n"
                "  --vcf-ref GENOME                only mappings whose target is of this genome (default any)\n"
                "  --vcf-query GENOME              only mappings whose query is of this genome; it names the sample column (default any, no sample)\n"
                "  --vcf-set kept|all              the records that are read (default kept)\n"
                "  --vcf-max-indel N               insertions and deletions up to N bases (default 10000; 0 = no limit)\n"
                "  --vcf-batch BYTES               CIGAR text per device call; k/m/g suffixes (default: from the device's memory; for tests)\n"
                "  --eqx FILE          write the records as PAF with every cg:Z: resolved to =/X against the FASTA (M ops told apart base by base,\n"
                "                      = and X ops checked), column 10 the exact matches, column 11 the block length; other tags are copied\n"
                "  --eqx-fasta FASTA               the sequences, matched to the PAF's names by exact name; once per file (needed)\n"
                "  --eqx-set kept|all              the records that are written (default kept)\n"
                "  --eqx-unresolved keep|drop      a record that cannot be resolved is copied unchanged, or left out (default keep)\n"
                "  --eqx-batch BYTES               CIGAR text and columns per device call; k/m/g suffixes (default: from the device's memory; for tests)\n"
                "  --maf FILE          write the records as MAF: per block `a score=`, the target's and the query's `s` line with their gapped bases (as\n"
                "                      the FASTA has them; the query reverse-complemented on '-') and an empty line; score is the block's aligned columns,\n"
                "                      no bases are compared\n"
                "  --maf-fasta FASTA               the sequences, matched to the PAF's names by exact name; once per file (needed)\n"
                "  --maf-set kept|all              the records that are written (default kept)\n"
                "  --maf-split-gap N               an I, D or N op of N bases or more ends a block and its bases are left out; k/m suffixes (default 0: one\n"
                "                                  block per record)\n"
                "  --maf-batch BYTES               CIGAR text and bases per device call; k/m/g suffixes (default: from the device's memory; for tests)\n"
                "  --divergence FILE   after the filter: one line per window of every sequence that carries an inter-genome mapping of the set --\n"
                "                      `sequence start end n aligned matches mismatches m_columns unaligned inserted mismatch_runs indels`, exact\n"
                "                      from the cg:Z: CIGARs (built on the device), empty windows included; integers only: column identity is\n"
                "                      matches / aligned, gap-compressed identity matches / (aligned + indels); - = standard error\n"
                "  --divergence-summary FILE  per sequence `length windows records entries` and the eight sums; records - entries is what the\n"
                "                      track does not see (a bad CIGAR, no tag)\n"
                "  --divergence-window N           bases per window; k/m/g suffixes (default 10k)\n"
                "  --divergence-axis query|target  the sequences the windows lie on (default query)\n"
                "  --divergence-genome NAME        only the mappings whose other side belongs to this genome (default: any other genome)\n"
                "  --divergence-set kept|all       the records that are read (default kept)\n"
                "  --divergence-batch BYTES        CIGAR text per device call; k/m/g suffixes (default: from the device's memory; for tests)\n"
                "  --lift-set kept|all       the mappings the rows of --lift go through (default kept)\n"
                "  --lift-axis query|target|both  regions lie on query sequences, target sequences or either (default both)\n"
                "  --lift-paf FILE     write every lifted region of --lift-regions as a PAF line of its own: the coordinates and the part of the\n"
                "                      record's cg:Z: CIGAR under the region, cut on the device; rn:Z: carries the BED label, ri:i: the record\n"
                "  --lift-paf-min-aligned N  leave out slices with fewer than N aligned columns (default 1)\n"
                "  --lift-batch BYTES  CIGAR text of the hit records per device call; k/m/g suffixes (default: from the device's memory; for tests)\n"
                "  --lift-hops N       walk the regions of --lift-regions through the mappings of --lift-set for up to N hops (1 .. 65535):\n"
                "                      what a region reaches through a third genome when no mapping joins the two directly\n"
                "  --lift-closure FILE `name start end label hop`: the disjoint pieces each region reaches, with the hop that found them\n"
                "                      (hop 0 = the region itself; no strand: a merged piece can come from both orientations)\n"
                "  --lift-closure-summary FILE  `label sequence start end pieces sequences genomes bases hops state` per region; state\n"
                "                      none = nothing beyond the region, closed = the walk ended by itself, cut = N ended it\n"
                "  --lift-min-length N a piece shorter than N bases is reported but not walked on (default 100): the projection is\n"
                "                      rounded outward, so the walk back through the same mapping reaches a few bases beyond the region\n"
                "Filter path of pangenome/sweepga on an MI355X (libsweepga_gpu.so).  No CPU fallback.");
      return 0;
    } else if (a.rfind("-", 0) == 0 && a != "-") die(2, "unknown flag " + a);
    else {
      input = a;
      inputs.push_back(a);
    }
  }
  if (joblist) return run_joblist(inputs, sparsify, mash_k, mash_s, threads_given ? (uint64_t)threads : 8, block_length, joblist_dir,
                                  output_file, device);
  if (components_path.empty() && (components_detailed || component_flag))
    die(2, "--components-detailed, --component-min-bases and --component-min-share need --components");
  if (sharing_path.empty() && sharing_detailed) die(2, "--sharing-detailed needs --sharing");
  if (mosaic_path.empty() && mosaic_share_path.empty() && mosaic_flag) die(2, "--mosaic-axis, --mosaic-set and --mosaic-by need --mosaic or --mosaic-share");
  const bool mosaic = !mosaic_path.empty() || !mosaic_share_path.empty();
  if (place_path.empty() && place_summary_path.empty() && place_flag)
    die(2, "--place-axis, --place-set and --place-min-bases need --place or --place-summary");
  const bool place = !place_path.empty() || !place_summary_path.empty();
  if (windows_path.empty() && windows_summary_path.empty() && windows_flag)
    die(2, "--window-size, --windows-axis and --windows-genome need --windows or --windows-summary");
  const bool windows = !windows_path.empty() || !windows_summary_path.empty();
  if (gaps_path.empty() && gaps_summary_path.empty() && gaps_flag) die(2, "--gaps-min-size needs --gaps or --gaps-summary");
  const bool gaps = !gaps_path.empty() || !gaps_summary_path.empty();
  if (dotplot_path.empty() && dotplot_layout_path.empty() && dotplot_flag)
    die(2, "--dotplot-size, --dotplot-query and --dotplot-target need --dotplot or --dotplot-layout");
  const bool lift = !lift_regions_path.empty();
  if (!lift && (!lift_paf_path.empty() || lift_paf_flag)) die(2, "--lift-paf, --lift-paf-min-aligned and --lift-batch need --lift-regions");
  if (lift_paf_path.empty() && lift_paf_flag) die(2, "--lift-paf-min-aligned and --lift-batch need --lift-paf");
  const bool lift_paf = !lift_paf_path.empty();
  if (!lift && (!lift_path.empty() || !lift_summary_path.empty() || lift_flag))
    die(2, "--lift, --lift-summary, --lift-set and --lift-axis need --lift-regions");
  if (!lift_hops && (!closure_path.empty() || !closure_summary_path.empty() || lift_min_length_flag))
    die(2, "--lift-closure, --lift-closure-summary and --lift-min-length need --lift-hops");
  if (lift_exact && (!lift || lift_path.empty())) die(2, "--lift-exact needs --lift-regions and --lift");
  if (ucsc_path.empty() && ucsc_flag) die(2, "--ucsc-chain-from, --ucsc-chain-set and --ucsc-chain-batch need --ucsc-chain");
  const bool ucsc = !ucsc_path.empty();
  const bool diffs = !diffs_path.empty() || !diffs_summary_path.empty();
  if (!diffs && diffs_flag) die(2, "--diffs-set, --diffs-kinds, --diffs-min-indel and --diffs-batch need --diffs or --diffs-summary");
  const bool vcf = !vcf_path.empty() || !vcf_summary_path.empty();
  if (!vcf && vcf_flag) die(2, "--vcf-fasta, --vcf-ref, --vcf-query, --vcf-set, --vcf-max-indel and --vcf-batch need --vcf or --vcf-summary");
  if (vcf && vcf_fasta_paths.empty()) die(2, "--vcf and --vcf-summary need --vcf-fasta: the bases are not in a PAF");
  swg_fasta* vcf_fasta = nullptr;
  if (vcf) {  // read now: an unreadable FASTA is a usage error, found before anything is begun
    std::vector<const char*> paths;
    for (const std::string& f : vcf_fasta_paths) paths.push_back(f.c_str());
    if (swg_fasta_open(paths.data(), (int)paths.size(), threads, &vcf_fasta) != SWG_OK) die(2, std::string("--vcf-fasta: ") + swg_fasta_last_error());
  }
  const bool eqx = !eqx_path.empty();
  if (!eqx && eqx_flag) die(2, "--eqx-fasta, --eqx-set, --eqx-unresolved and --eqx-batch need --eqx");
  if (eqx && eqx_fasta_paths.empty()) die(2, "--eqx needs --eqx-fasta: the bases are not in a PAF");
  swg_fasta* eqx_fasta = nullptr;
  if (eqx) {  // read now: an unreadable FASTA is a usage error, found before anything is begun
    std::vector<const char*> paths;
    for (const std::string& f : eqx_fasta_paths) paths.push_back(f.c_str());
    if (swg_fasta_open(paths.data(), (int)paths.size(), threads, &eqx_fasta) != SWG_OK) die(2, std::string("--eqx-fasta: ") + swg_fasta_last_error());
  }
  const bool maf = !maf_path.empty();
  if (!maf && maf_flag) die(2, "--maf-fasta, --maf-set, --maf-split-gap and --maf-batch need --maf");
  if (maf && maf_fasta_paths.empty()) die(2, "--maf needs --maf-fasta: the bases are not in a PAF");
  swg_fasta* maf_fasta = nullptr;
  if (maf) {  // read now: an unreadable FASTA is a usage error, found before anything is begun
    std::vector<const char*> paths;
    for (const std::string& f : maf_fasta_paths) paths.push_back(f.c_str());
    if (swg_fasta_open(paths.data(), (int)paths.size(), threads, &maf_fasta) != SWG_OK) die(2, std::string("--maf-fasta: ") + swg_fasta_last_error());
  }
  const bool divergence = !divergence_path.empty() || !divergence_summary_path.empty();
  if (!divergence && divergence_flag)
    die(2, "--divergence-window, --divergence-axis, --divergence-genome, --divergence-set and --divergence-batch need --divergence or --divergence-summary");
  if (lift_hops && !lift) die(2, "--lift-hops needs --lift-regions");
  if (lift_hops && closure_path.empty() && closure_summary_path.empty()) die(2, "--lift-hops needs --lift-closure or --lift-closure-summary");
  if (lift && lift_path.empty() && lift_summary_path.empty() && !lift_hops && !lift_paf) die(2, "--lift-regions needs --lift or --lift-summary");
  const bool lift_once = lift && (!lift_path.empty() || !lift_summary_path.empty());  // the one-hop reports are asked for
  if (lift) {  // read now: an unreadable BED is a usage error, found before anything is begun
    FILE* f = std::fopen(lift_regions_path.c_str(), "rb");
    if (!f) die(2, "cannot open " + lift_regions_path + ": " + std::strerror(errno));
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) lift_bed.append(buf, got);
    const bool failed = std::ferror(f) != 0;
    std::fclose(f);
    if (failed) die(2, "cannot read " + lift_regions_path);
    // a malformed BED is a usage error too: parsed here against a handle without records, which needs no device
    char marker = 0;
    char* text[2] = {nullptr, &marker};
    uint64_t len[2] = {0, 0};
    const uint8_t none = 0;
    swg_paf* empty = nullptr;
    if (swg_paf_open_buffer("", 0, 1, &empty) != SWG_OK) die(3, swg_paf_last_error());
    const int rc = swg_paf_lift(nullptr, empty, &none, lift_bed.data(), lift_bed.size(), lift_set, lift_axes, text, len);
    swg_paf_close(empty);
    if (rc != SWG_OK) die(2, std::string("--lift-regions: ") + swg_alnstats_last_error());
    swg_free(text[1]);
  }
  dot_view.query_prefix = dotplot_query.empty() ? nullptr : dotplot_query.c_str();
  dot_view.target_prefix = dotplot_target.empty() ? nullptr : dotplot_target.c_str();
  if (input.empty()) die(2, "usage: sweepga-gpu <in.paf> [--output-file out.paf] [filter flags]   (--help)");

  if (!no_filter && !bad_sparsify.empty()) die(1, "--sparsify '" + bad_sparsify + "' is not valid for post-alignment PAF/1aln filtering");
  swg_config cfg{};
  if (!parse_filter_mode(num_mappings, &cfg.mapping_filter_mode, &cfg.mapping_max_per_query, &cfg.mapping_max_per_target)) return 1;
  if (!parse_filter_mode(scaffold_filter, &cfg.scaffold_filter_mode, &cfg.scaffold_max_per_query, &cfg.scaffold_max_per_target)) return 1;
  cfg.scoring_function = parse_scoring(scoring);
  cfg.min_block_length = block_length;
  cfg.overlap_threshold = overlap;
  cfg.scaffold_gap = scaffold_jump;
  cfg.min_scaffold_length = scaffold_mass;
  cfg.scaffold_overlap_threshold = scaffold_overlap;
  cfg.scaffold_max_deviation = scaffold_dist;
  cfg.keep_self = keep_self;
  cfg.scaffolds_only = scaffolds_only;
  // identity thresholds: plain numbers are checked now, "aniN" forms after the ANI pre-pass (main.rs:3571-3595)
  auto lower = [](std::string v) {
    for (auto& c : v)
      if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
    return v;
  };
  const bool need_ani = lower(min_identity).find("ani") != std::string::npos || lower(min_scaffold_identity).find("ani") != std::string::npos;
  auto set_identities = [&](double ani_percentile) {
    if (swg_parse_identity_value(min_identity.c_str(), ani_percentile, &cfg.min_identity) != SWG_OK)
      die(2, std::string("bad --min-aln-identity: ") + swg_paf_last_error());
    if (min_scaffold_identity.empty()) cfg.min_scaffold_identity = cfg.min_identity;
    else if (swg_parse_identity_value(min_scaffold_identity.c_str(), ani_percentile, &cfg.min_scaffold_identity) != SWG_OK)
      die(2, std::string("bad --min-scaffold-identity: ") + swg_paf_last_error());
  };
  if (!need_ani) set_identities(-1.0);

  // ---- HIP start-up (~0.1 s), device memory for an input of this size and the library's code objects (swg_warmup) are
  // prepared on a thread of their own while the host threads read and parse the input
  if (devices.empty()) devices.push_back(device);
  uint64_t records_hint = 0;
  {
    // lines in the file ~ file size / the average line length of its first 256 KB (real PAFs with cg:Z: / tp:A: tags run
    // 150-250 bytes a line, bare ones ~90: a fixed guess over-reserves device memory for the whole run); compressed inputs
    // are not guessed
    struct stat sb;
    const bool gz = input.size() > 3 && (input.rfind(".gz") == input.size() - 3 || input.rfind(".bgz") == input.size() - 4);
    if (input != "-" && !gz && stat(input.c_str(), &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
      double per_line = 200.0;
      if (FILE* f = fopen(input.c_str(), "rb")) {
        std::vector<char> head(size_t(256) << 10);
        const size_t got = fread(head.data(), 1, head.size(), f);
        fclose(f);
        size_t nl = 0, last = 0;
        for (size_t i = 0; i < got; ++i)
          if (head[i] == '\n') {
            ++nl;
            last = i + 1;
          }
        if (nl) per_line = (double)last / (double)nl;
      }
      records_hint = (uint64_t)((double)sb.st_size / per_line * 1.02) + 1;
    }
  }
  std::vector<swg_ctx*> ctxs;
  int init_rc = SWG_OK;
  std::string init_err;
  double create_ms = 0.0, warm_ms = 0.0;
  std::thread gpu_init([&] {
    if (no_filter && breadth_path.empty() && components_path.empty() && lost_path.empty() && covered_path.empty() && sharing_path.empty() &&
        sharing_bed_path.empty() && dotplot_path.empty() && !lift && !mosaic && !place && !windows && !ucsc && !diffs && !divergence && !vcf && !eqx && !maf)
      return;  // (--no-filter opens a device only for these reports)
    for (int d : devices) {
      if (no_filter && !ctxs.empty()) break;  // (... and the report runs on the first context)
      swg_ctx* c = nullptr;
      const auto c0 = std::chrono::steady_clock::now();
      init_rc = swg_create(d, &c);
      create_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
      if (init_rc != SWG_OK) {
        init_err = swg_last_error(nullptr);  // thread-local: read it on this thread
        return;
      }
      ctxs.push_back(c);
      const auto w0 = std::chrono::steady_clock::now();
      // best effort: a failure here (e.g. no room for the speculative reservation) shows up again, with its own message, in
      // the filter call, which sizes itself; SWG_DEBUG prints this one too
      // (--no-filter --breadth runs no filter: the report's call sizes its own, smaller arena)
      if (no_filter) continue;
      if (swg_warmup(c, records_hint / devices.size(), 4096, cfg.scaffold_gap != 0) != SWG_OK && getenv("SWG_DEBUG"))
        fprintf(stderr, "[sweepga-gpu] warm-up on device %d failed (ignored): %s\n", d, swg_last_error(c));
      warm_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    }
  });

  // ---- open_paf_input + extract_metadata (paf_filter.rs:292-376), multi-threaded in libsweepga_gpu.so
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  swg_paf* paf = nullptr;
  // the parse leaves a few hardware threads to the device start-up that runs beside it (the HIP runtime's own threads and
  // the warm-up: with every hardware thread parsing, context creation took 0.4-1.0 s instead of 0.1 s at 10^8 lines)
  // and no more than 64: the parse of 10^8 lines takes 0.62 s on 64 threads of the GPU box's 256-thread host, 0.91 s on 128
  // and 1.29 s on 248 (first-touch page faults of ~7 GB of columns in one address space: more threads get in each other's way)
  int parse_threads = threads;
  if (parse_threads <= 0 && !no_filter) {
    const unsigned hc = std::thread::hardware_concurrency();
    if (hc > 16) parse_threads = (int)std::min(hc - 8, 64u);
  }
  if (swg_paf_open(input.c_str(), parse_threads, &paf) != SWG_OK) {
    const std::string msg = swg_paf_last_error();
    gpu_init.join();
    die(2, msg);
  }
  // --vcf-ref / --vcf-query name genomes of this file: an unknown name is a usage error, found before the filter runs and before any
  // report is written
  if (vcf && swg_paf_records(paf)->n) {
    for (const std::string* name : {&vcf_ref, &vcf_query}) {
      if (name->empty()) continue;
      bool found = false;
      for (uint32_t g = 0, G = swg_paf_num_genomes_two(paf); g < G && !found; ++g) {
        const std::string have = swg_paf_genome_two_prefix(paf, g);
        found = have == *name || have == *name + "#";
      }
      if (!found) {
        gpu_init.join();
        die(2, std::string(name == &vcf_ref ? "--vcf-ref" : "--vcf-query") + ": unknown genome '" + *name + "'");
      }
    }
  }
  // --breadth reads 32-bit columns (swg_paf_breadth): refused here, not after a whole filter run and ahead of the output
  if (!breadth_path.empty() && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {
    gpu_init.join();
    die(3, "--breadth: the file has a value >= 2^32, its columns are rebased: breadth of 64-bit columns is not supported");
  }
  if (!components_path.empty() && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--components: the file has a value >= 2^32, its columns are rebased: components of 64-bit columns are not supported");
  }
  if ((!lost_path.empty() || !covered_path.empty()) && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--lost / --covered: the file has a value >= 2^32, its columns are rebased: intervals of 64-bit columns are not supported");
  }
  if ((!sharing_path.empty() || !sharing_bed_path.empty()) && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--sharing: the file has a value >= 2^32, its columns are rebased: sharing of 64-bit columns is not supported");
  }
  if (mosaic && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--mosaic: the file has a value >= 2^32, its columns are rebased: the mosaic of 64-bit columns is not supported");
  }
  if (place && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--place: the file has a value >= 2^32, its columns are rebased: the placement of 64-bit columns is not supported");
  }
  if (windows && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--windows: the file has a value >= 2^32, its columns are rebased: the windows of 64-bit columns are not supported");
  }
  if (divergence && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--divergence: the file has a value >= 2^32, its columns are rebased: the divergence of 64-bit columns is not supported");
  }
  if ((!dotplot_path.empty() || !dotplot_layout_path.empty()) && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--dotplot: the file has a value >= 2^32, its columns are rebased: a dot plot of 64-bit columns is not supported");
  }
  if (lift) {
    if (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0)) {  // (likewise)
      gpu_init.join();
      die(3, "--lift: the file has a value >= 2^32, its columns are rebased: a lift through 64-bit columns is not supported");
    }
  }
  if (!blocks_path.empty() && !no_filter && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--blocks: the file has a value >= 2^32, its columns are rebased: blocks of 64-bit columns are not supported");
  }
  if (gaps && (swg_paf_seq_offsets(paf) || swg_paf_record_offsets(paf, 0))) {  // (likewise)
    gpu_init.join();
    die(3, "--gaps: the file has a value >= 2^32, its columns are rebased: gaps of 64-bit columns are not supported");
  }
  const std::string out_path = output_file.empty() ? "-" : output_file;
  const swg_records* r = swg_paf_records(paf);
  uint64_t n = r->n;
  if (no_filter) {  // main.rs:3461-3473: every line, newline-normalised, ALWAYS to stdout (--output-file is not consulted)
    const char* text;
    uint64_t len;
    swg_paf_text(paf, &text, &len);
    FILE* out = stdout;
    for (uint64_t pos = 0; pos < len;) {
      const void* nl = std::memchr(text + pos, '\n', len - pos);
      const uint64_t end = nl ? (uint64_t)((const char*)nl - text) : len;
      uint64_t ll = end - pos;
      if (nl && ll && text[pos + ll - 1] == '\r') --ll;
      std::fwrite(text + pos, 1, ll, out);
      std::fputc('\n', out);
      pos = end + 1;
    }
    if (!stats_path.empty()) {  // no device is needed for this report: the host tool's statistics of the same lines, twice
      std::fflush(out);
      swg_alnstats* sa = nullptr;
      if (swg_alnstats_open_buffer(text, len, threads, &sa) != SWG_OK) die(3, std::string("--stats: ") + swg_alnstats_last_error());
      write_stats_report(stats_path, sa, sa, input, out_path, stats_detailed);
      swg_alnstats_close(sa);
    }
    gpu_init.join();
    if (!breadth_path.empty()) {  // nothing is dropped: the kept rows equal the all rows
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_breadth_report(breadth_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), breadth_detailed);
    }
    if (!blocks_path.empty()) {  // no filter, no chains
      std::fflush(out);
      write_blocks(blocks_path, nullptr, paf, nullptr, nullptr);
    }
    if (gaps) {  // no filter, no chains: the header lines
      std::fflush(out);
      write_gaps(gaps_path, gaps_summary_path, nullptr, paf, nullptr, nullptr, (uint32_t)gaps_min_size);
    }
    if (!components_path.empty()) {  // nothing is dropped: every record takes part
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      write_components(components_path, ctxs.empty() ? nullptr : ctxs[0], paf, nullptr, component_par, components_detailed);
    }
    if (!lost_path.empty() || !covered_path.empty()) {  // nothing is dropped: nothing is lost, what is covered is what all records cover
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_intervals(lost_path, covered_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data());
    }
    if (!sharing_path.empty() || !sharing_bed_path.empty()) {  // nothing is dropped: the kept columns equal the all columns
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_sharing(sharing_path, sharing_bed_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), sharing_detailed);
    }
    if (mosaic) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_mosaic(mosaic_path, mosaic_share_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), mosaic_axis, mosaic_set, mosaic_by_length);
    }
    if (place) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_place(place_path, place_summary_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), place_axis, place_set, place_min_bases);
    }
    if (windows) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_windows(windows_path, windows_summary_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), windows_axis, (uint32_t)window_size, windows_genome);
    }
    if (!dotplot_path.empty() || !dotplot_layout_path.empty()) {  // nothing is dropped: the kept planes equal the all planes
      std::fflush(out);
      if (n && !dotplot_path.empty() && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_dotplot(dotplot_path, dotplot_layout_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), dot_view);
    }
    if (lift) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      if (lift_once) write_lift(lift_path, lift_summary_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), lift_bed, lift_set, lift_axes, lift_exact, quiet);
      if (lift_hops)
        write_lift_closure(closure_path, closure_summary_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), lift_bed, lift_set, lift_axes,
                           (uint32_t)lift_hops, (uint32_t)lift_min_length);
      if (lift_paf)
        write_lift_paf(lift_paf_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), lift_bed, lift_set, lift_axes, (uint32_t)lift_paf_min_aligned,
                       lift_batch, quiet);
    }
    if (ucsc) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_ucsc_chain(ucsc_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), ucsc_set, ucsc_from, ucsc_batch, quiet);
    }
    if (diffs) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_diffs(diffs_path, diffs_summary_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), diffs_set, diffs_kinds, (uint32_t)diffs_min_indel,
                  diffs_batch, quiet);
    }
    if (vcf) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_vcf(vcf_path, vcf_summary_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), vcf_fasta, vcf_set, vcf_ref, vcf_query, (uint32_t)vcf_max_indel,
                vcf_batch, quiet);
      swg_fasta_close(vcf_fasta);
    }
    if (eqx) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_eqx(eqx_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), eqx_fasta, eqx_set, eqx_unresolved, eqx_batch, quiet);
      swg_fasta_close(eqx_fasta);
    }
    if (maf) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_maf(maf_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), maf_fasta, maf_set, (uint32_t)maf_split_gap, maf_batch, quiet);
      swg_fasta_close(maf_fasta);
    }
    if (divergence) {  // nothing is dropped: kept = all
      std::fflush(out);
      if (n && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
      const std::vector<uint8_t> every(n ? n : 1, 1);
      write_divergence(divergence_path, divergence_summary_path, ctxs.empty() ? nullptr : ctxs[0], paf, every.data(), divergence_set, divergence_axis,
                       (uint32_t)divergence_window, divergence_genome, divergence_batch, quiet);
    }
    for (swg_ctx* c : ctxs) swg_destroy(c);
    swg_paf_close(paf);
    return 0;
  }
  const auto t1 = clk::now();

  // ---- ANI pre-pass over the input when a threshold asks for it
  gpu_init.join();
  const auto t1b = clk::now();  // what the device start-up took beyond the read
  if ((n || need_ani) && init_rc != SWG_OK) die(3, "no usable GPU: " + init_err);
  swg_ctx* ctx = ctxs.empty() ? nullptr : ctxs[0];
  double ani_percentile = -1.0, ani_ms = 0.0;
  if (need_ani) {
    int kind = SWG_ANI_NPERCENTILE, nsort = SWG_NSORT_IDENTITY;
    double pct = 50.0;
    if (!swg_parse_ani_method(ani_method_s.c_str(), &kind, &pct, &nsort)) {  // unknown method: n50-identity
      kind = SWG_ANI_NPERCENTILE;
      pct = 50.0;
      nsort = SWG_NSORT_IDENTITY;
    }
    const auto ta = clk::now();
    if (swg_paf_ani_stats(ctx, paf, kind, pct, nsort, threads, &ani_percentile) != SWG_OK) die(3, std::string("ANI pre-pass failed: ") + swg_paf_last_error());
    ani_ms = std::chrono::duration<double, std::milli>(clk::now() - ta).count();
  }
  if (need_ani) set_identities(ani_percentile);
  if (need_ani && !quiet) std::fprintf(stderr, "[sweepga-gpu] ANI pre-pass (%s): median %.6f in %.1f ms\n", ani_method_s.c_str(), ani_percentile, ani_ms);

  // ---- tree sparsification of the input (src/main.rs:3640-3688).  The reference filters a temporary tree-filtered file; here the
  // sparsification is a keep flag per record of the handle that is already open, the filter runs on the kept subset and answers
  // in the handle's record indices, and the writer takes the full-length status: no second text buffer, no second parse.  A
  // dropped record has status 0 and is not written, so the output is the filter's output on the sparsified text.
  std::vector<uint8_t> tree_keep;
  const auto t1c = clk::now();
  if (!tree_sparsify.empty()) {
    tree_keep.resize(n ? n : 1);
    uint64_t n_tree = 0;
    int route = SWG_TREE_ROUTE_DEVICE;
    if (swg_paf_tree_select(ctx, paf, tree_near, tree_far, tree_rand, threads, tree_keep.data(), &n_tree, &route) != SWG_OK)
      die(2, std::string("tree sparsification failed: ") + (ctx ? swg_last_error(ctx) : ""));
    if (!quiet)
      std::fprintf(stderr, "[sweepga-gpu] --sparsify %s: %s, %llu records -> %llu kept by the sparsification, %.1f ms\n", tree_sparsify.c_str(),
                   route == SWG_TREE_ROUTE_DEVICE ? "device mask" : "text fall-back", (unsigned long long)n, (unsigned long long)n_tree,
                   std::chrono::duration<double, std::milli>(clk::now() - t1c).count());
  }
  const uint8_t* const keep_mask = tree_sparsify.empty() ? nullptr : tree_keep.data();

  // ---- apply_filters on the GPU
  // result columns: uninitialised storage (the filter writes every entry; zero-filling 0.5 GB on this thread first cost
  // ~85 ms per 10^8 records), 2 MB-aligned and marked for huge pages like the ingest's columns
  auto alloc_col = [&](size_t bytes) -> void* {
    void* p = nullptr;
    const size_t two_mb = size_t(2) << 20;
    if (bytes >= (size_t(8) << 20) && posix_memalign(&p, two_mb, (bytes + two_mb - 1) & ~(two_mb - 1)) == 0)
      madvise(p, bytes, MADV_HUGEPAGE);
    else
      p = std::calloc(bytes ? bytes : 1, 1);
    if (!p) die(3, "out of host memory for the result columns");
    return p;
  };
  struct View8 { uint8_t* p; uint8_t* data() const { return p; } } status{static_cast<uint8_t*>(alloc_col(n ? n : 1))};
  struct View32 { uint32_t* p; uint32_t* data() const { return p; } } chain{static_cast<uint32_t*>(alloc_col((n ? n : 1) * sizeof(uint32_t)))};
  swg_stats st{};
  if (n) {
    // no dv:f: override anywhere: identity = matches / max(block length, 1) for every record, which the device evaluates
    // itself -- the column (8 of 47 bytes per record) stays on the host
    swg_records rr = *r;
    if (swg_paf_identity_is_derived(paf)) rr.identity = nullptr;
    // The result columns are not cleared (posix_memalign above): every filter path must write every entry.  SWG_DEBUG checks
    // that it does: the columns start as 0xff (no status, no chain number of a real result has that byte pattern in every
    // byte: statuses are 0..3, chain numbers stay below 2^31) and none of it may be left.
    const bool poison = std::getenv("SWG_DEBUG") != nullptr;
    if (poison) {
      std::memset(status.data(), 0xff, n);
      std::memset(chain.data(), 0xff, n * sizeof(uint32_t));
    }
    // (keep_mask == NULL: swg_filter / swg_filter_multi themselves)
    const int rc = ctxs.size() > 1 ? swg_filter_subset_multi(ctxs.data(), (int)ctxs.size(), &rr, keep_mask, &cfg, status.data(), chain.data(), &st)
                                   : swg_filter_subset(ctx, &rr, keep_mask, &cfg, status.data(), chain.data(), &st);
    if (rc != SWG_OK) die(3, std::string("filter failed: ") + swg_last_error(ctx));
    if (poison) {
      for (uint64_t i = 0; i < n; ++i)
        if (status.data()[i] == 0xff || chain.data()[i] == 0xffffffffu)
          die(3, "internal: the filter left record " + std::to_string(i) + " of the result columns unwritten");
    }
  }
  const auto t2 = clk::now();

  // ---- --stats: before / after from the columns and the status the filter left, ahead of the write
  if (!stats_path.empty()) {
    swg_alnstats *sa = nullptr, *sk = nullptr;
    // (with --sparsify too: "before" is the whole input, "after" what is written -- one call on the one handle)
    if (swg_paf_alnstats(ctx, paf, status.data(), &sa, &sk) != SWG_OK) die(3, std::string("--stats: ") + swg_alnstats_last_error());
    write_stats_report(stats_path, sa, sk, input, out_path, stats_detailed);
    if (!quiet) {
      const double ms = std::chrono::duration<double, std::milli>(clk::now() - t2).count();
      std::fprintf(stderr, "[sweepga-gpu] --stats: %.1f ms\n", ms);
    }
    swg_alnstats_close(sa);
    swg_alnstats_close(sk);
  }
  // ---- --breadth: on the first context (with --sparsify: "all" is the whole input, "kept" what is written)
  if (!breadth_path.empty()) {
    const auto tb = clk::now();
    write_breadth_report(breadth_path, ctx, paf, status.data(), breadth_detailed);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --breadth: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --blocks: on the first context, from the (merged) status and chain the filter left; records that a sparsification dropped
  // carry chain 0 and take no part
  if (!blocks_path.empty()) {
    const auto tb = clk::now();
    write_blocks(blocks_path, ctx, paf, status.data(), chain.data());
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --blocks: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --place / --place-summary: on the first context, under the merged status (with --sparsify, dropped records have status 0)
  if (place) {
    const auto tb = clk::now();
    write_place(place_path, place_summary_path, ctx, paf, status.data(), place_axis, place_set, place_min_bases);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --place: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --windows / --windows-summary: likewise, both from one device call
  if (windows) {
    const auto tb = clk::now();
    write_windows(windows_path, windows_summary_path, ctx, paf, status.data(), windows_axis, (uint32_t)window_size, windows_genome);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --windows: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --gaps / --gaps-summary: likewise, both from one device call
  if (gaps) {
    const auto tb = clk::now();
    write_gaps(gaps_path, gaps_summary_path, ctx, paf, status.data(), chain.data(), (uint32_t)gaps_min_size);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --gaps: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --components: on the first context, from the (merged) status the filter left
  if (!components_path.empty()) {
    const auto tb = clk::now();
    write_components(components_path, ctx, paf, status.data(), component_par, components_detailed);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --components: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --lost / --covered: on the first context (with --sparsify: "all" is the whole input, "kept" what is written)
  if (!lost_path.empty() || !covered_path.empty()) {
    const auto tb = clk::now();
    write_intervals(lost_path, covered_path, ctx, paf, status.data());
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --lost / --covered: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --sharing / --sharing-bed: on the first context (with --sparsify: "all" is the whole input, "kept" what is written)
  if (!sharing_path.empty() || !sharing_bed_path.empty()) {
    const auto tb = clk::now();
    write_sharing(sharing_path, sharing_bed_path, ctx, paf, status.data(), sharing_detailed);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --sharing: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --mosaic / --mosaic-share: on the first context (with --sparsify: "all" is the whole input, "kept" what is written)
  if (mosaic) {
    const auto tb = clk::now();
    write_mosaic(mosaic_path, mosaic_share_path, ctx, paf, status.data(), mosaic_axis, mosaic_set, mosaic_by_length);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --mosaic: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --dotplot / --dotplot-layout: on the first context (with --sparsify: "all" is the whole input, "kept" what is written)
  if (!dotplot_path.empty() || !dotplot_layout_path.empty()) {
    const auto tb = clk::now();
    write_dotplot(dotplot_path, dotplot_layout_path, ctx, paf, status.data(), dot_view);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --dotplot: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --lift / --lift-summary: on the first context (with --sparsify: "all" is the whole input, "kept" what is written)
  if (lift) {
    const auto tb = clk::now();
    if (lift_once) write_lift(lift_path, lift_summary_path, ctx, paf, status.data(), lift_bed, lift_set, lift_axes, lift_exact, quiet);
    if (lift_once && !quiet) std::fprintf(stderr, "[sweepga-gpu] --lift: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
    if (lift_hops) {  // --lift-hops: the transitive lift through the same set and axes
      const auto tc = clk::now();
      write_lift_closure(closure_path, closure_summary_path, ctx, paf, status.data(), lift_bed, lift_set, lift_axes, (uint32_t)lift_hops,
                         (uint32_t)lift_min_length);
      if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --lift-hops: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tc).count());
    }
    if (lift_paf) {  // --lift-paf: every lifted region as an alignment of its own
      const auto tc = clk::now();
      write_lift_paf(lift_paf_path, ctx, paf, status.data(), lift_bed, lift_set, lift_axes, (uint32_t)lift_paf_min_aligned, lift_batch, quiet);
      if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --lift-paf: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tc).count());
    }
  }
  // ---- --ucsc-chain: on the first context, the records in batches of bounded CIGAR text
  if (ucsc) {
    const auto tb = clk::now();
    write_ucsc_chain(ucsc_path, ctx, paf, status.data(), ucsc_set, ucsc_from, ucsc_batch, quiet);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --ucsc-chain: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --diffs / --diffs-summary: on the first context, the records in batches of bounded CIGAR text
  if (diffs) {
    const auto tb = clk::now();
    write_diffs(diffs_path, diffs_summary_path, ctx, paf, status.data(), diffs_set, diffs_kinds, (uint32_t)diffs_min_indel, diffs_batch, quiet);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --diffs: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --vcf / --vcf-summary: likewise, the bases on the device once, one stable device sort after the last batch
  if (vcf) {
    const auto tb = clk::now();
    write_vcf(vcf_path, vcf_summary_path, ctx, paf, status.data(), vcf_fasta, vcf_set, vcf_ref, vcf_query, (uint32_t)vcf_max_indel, vcf_batch, quiet);
    swg_fasta_close(vcf_fasta);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --vcf: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --eqx: likewise, the bases on the device once, one device pass per batch
  if (eqx) {
    const auto tb = clk::now();
    write_eqx(eqx_path, ctx, paf, status.data(), eqx_fasta, eqx_set, eqx_unresolved, eqx_batch, quiet);
    swg_fasta_close(eqx_fasta);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --eqx: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --maf: likewise, the bases on the device once, one device pass per batch
  if (maf) {
    const auto tb = clk::now();
    write_maf(maf_path, ctx, paf, status.data(), maf_fasta, maf_set, (uint32_t)maf_split_gap, maf_batch, quiet);
    swg_fasta_close(maf_fasta);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --maf: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  // ---- --divergence / --divergence-summary: likewise, one device call per batch over all records
  if (divergence) {
    const auto tb = clk::now();
    write_divergence(divergence_path, divergence_summary_path, ctx, paf, status.data(), divergence_set, divergence_axis, (uint32_t)divergence_window,
                     divergence_genome, divergence_batch, quiet);
    if (!quiet) std::fprintf(stderr, "[sweepga-gpu] --divergence: %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tb).count());
  }
  const auto t2s = clk::now();

  // ---- write_filtered_output (paf_filter.rs:1689-1726): input order, original bytes + tags
  uint64_t kept = 0;
  if (swg_paf_write(paf, out_path.c_str(), status.data(), chain.data(), threads, &kept) != SWG_OK) die(2, swg_paf_last_error());
  const auto t3 = clk::now();
  if (!quiet) {
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    double load_ms, parse_ms;
    swg_paf_timing(paf, &load_ms, &parse_ms);
    std::fprintf(stderr,
                 "[sweepga-gpu] %llu records -> %llu kept | read %.1f ms (load %.1f, parse %.1f), filter %.1f ms (device %.1f, h2d %.1f, "
                 "d2h %.1f), write %.1f ms | device start-up %.1f ms beside the read (create %.1f, warm-up %.1f), %.1f ms waited for\n",
                 (unsigned long long)n, (unsigned long long)kept, ms(t0, t1), load_ms, parse_ms, ms(t1b, t2), st.device_ms, st.h2d_ms,
                 st.d2h_ms, ms(t2s, t3), create_ms + warm_ms, create_ms, warm_ms, ms(t1, t1b));
  }
  if (!quiet) {
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "[sweepga-gpu] main() %.1f ms\n", ms(t_main, clk::now()));
  }
  // The output is written and closed.  Unmapping a multi-GB input, freeing the columns and the HIP runtime's
  // exit handlers cost ~0.1 s that buy nothing in a process about to end: leave all of it to the kernel.
  std::fflush(stdout);
  std::fflush(stderr);
  (void)paf;
  (void)ctxs;
  _exit(0);
}
