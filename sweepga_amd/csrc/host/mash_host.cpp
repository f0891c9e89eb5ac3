// Haplotype pair selection and the `--joblist` command list (host side of csrc/swg_mash.hip):
//
//   haplotype key ...... extract_pansn_key(name, Haplotype)         src/pansn.rs:58-86
//   groups ............. group_indices_by_pansn: BTreeMap key order   src/pansn.rs:112-123
//   haplotype sketch ... merge_sketches: concat, sort, dedup, truncate src/knn_graph.rs:568-582
//   selection .......... select_pairs / select_pairs_from_sketches,  src/knn_graph.rs:243-393, 400-560
//                        build_knn_graph (stable sorts by partial_cmp), generate_random_pairs (on the device)
//   jobs ............... pansn_joblist_jobs + write_wfmash_pansn_commands   src/main.rs:848-960, src/joblist.rs:102-145
//
// Jobs are collapsed to (min key, max key) haplotype pairs plus every haplotype's self pair, in BTreeSet order.  Because
// haplotype indices follow the key order, that is the order of (i, j) index pairs.  An input without PanSN structure (as
// many haplotypes as contigs) makes the reference fall back to per-file `sweepga` self-invocations, which this library
// does not emit: SWG_ERR_UNSUPPORTED.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

namespace {

struct Strategy {
  enum Kind { None, Auto, Random, Connectivity, Tree, Wfmash } kind = None;
  double f = 0.0;  // Random fraction, Connectivity probability, Tree random fraction
  uint64_t near = 0, far = 0;
};

bool parse_f64(const std::string& s, double* out) {  // str::parse::<f64> (no leading / trailing space, no hex)
  if (s.empty() || s.find_first_of(" \t\n\r\f\vxX(") != std::string::npos) return false;
  char* e = nullptr;
  const double v = std::strtod(s.c_str(), &e);
  if (e == s.c_str() || *e) return false;
  *out = v;
  return true;
}
bool parse_usize(const std::string& s, uint64_t* out) {  // str::parse::<usize>
  size_t i = (!s.empty() && s[0] == '+') ? 1 : 0;
  if (i >= s.size()) return false;
  uint64_t v = 0;
  for (; i < s.size(); ++i) {
    if (s[i] < '0' || s[i] > '9') return false;
    const uint64_t d = (uint64_t)(s[i] - '0');
    if (v > (UINT64_MAX - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = v;
  return true;
}

// SparsificationStrategy::from_str, src/knn_graph.rs:59-160
bool parse_strategy(const std::string& s, Strategy* st) {
  double f;
  if (parse_f64(s, &f)) {
    if (!(f > 0.0 && f <= 1.0)) return false;
    *st = {Strategy::Random, f};
    return true;
  }
  if (s == "none" || s == "all") return *st = {Strategy::None}, true;
  if (s == "auto") return *st = {Strategy::Auto}, true;
  if (s.rfind("random:", 0) == 0) {
    if (!parse_f64(s.substr(7), &f) || !(f > 0.0 && f <= 1.0)) return false;
    *st = {Strategy::Random, f};
    return true;
  }
  if (s.rfind("giant:", 0) == 0 || s.rfind("connectivity:", 0) == 0) {
    if (!parse_f64(s.substr(s.find(':') + 1), &f) || !(f > 0.0 && f < 1.0)) return false;
    *st = {Strategy::Connectivity, f};
    return true;
  }
  if (s.rfind("tree:", 0) == 0 || s.rfind("knn:", 0) == 0) {
    const std::string body = s.substr(s.find(':') + 1);
    std::vector<std::string> parts;
    for (size_t a = 0;;) {
      const size_t c = body.find(':', a);
      parts.push_back(body.substr(a, c == std::string::npos ? std::string::npos : c - a));
      if (c == std::string::npos) break;
      a = c + 1;
    }
    if (parts.size() > 3) return false;
    Strategy t{Strategy::Tree};
    if (!parse_usize(parts[0], &t.near)) return false;
    if (parts.size() > 1 && !parse_usize(parts[1], &t.far)) return false;
    if (parts.size() > 2 && !parse_f64(parts[2], &t.f)) return false;
    if (t.near == 0 && t.far == 0) return false;
    if (!(t.f >= 0.0 && t.f <= 1.0)) return false;
    *st = t;
    return true;
  }
  if (s.rfind("wfmash:", 0) == 0) {
    const std::string v = s.substr(7);
    if (v != "auto" && (!parse_f64(v, &f) || !(f > 0.0 && f <= 1.0))) return false;
    *st = {Strategy::Wfmash};
    return true;
  }
  return false;
}

bool needs_sketches(const Strategy& st) { return st.kind == Strategy::Auto || st.kind == Strategy::Connectivity || st.kind == Strategy::Tree; }

using Pairs = std::vector<std::pair<uint64_t, uint64_t>>;

void all_pairs(uint64_t n, Pairs* out) {
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t j = i + 1; j < n; ++j) out->emplace_back(i, j);
}

int random_pairs(swg_ctx* ctx, uint64_t n, double fraction, Pairs* out) {  // generate_random_pairs, knn_graph.rs:362-386
  if (n < 2) return SWG_OK;
  const uint64_t wpr = (n + 63) / 64;
  const uint64_t rows_per = std::max<uint64_t>(1, (uint64_t(1) << 24) / wpr);
  std::vector<uint64_t> mask;
  for (uint64_t r0 = 0; r0 < n; r0 += rows_per) {
    const uint64_t r1 = std::min(n, r0 + rows_per);
    mask.assign((r1 - r0) * wpr, 0);
    const int rc = swg_mash_random_pairs(ctx, n, fraction, r0, r1, mask.data());
    if (rc != SWG_OK) return rc;
    for (uint64_t i = r0; i < r1; ++i)
      for (uint64_t w = 0; w < wpr; ++w)
        for (uint64_t m = mask[(i - r0) * wpr + w]; m; m &= m - 1) out->emplace_back(i, w * 64 + (uint64_t)__builtin_ctzll(m));
  }
  return SWG_OK;
}

void knn(const double* d, uint64_t n, uint64_t kk, bool farthest, Pairs* out) {  // build_knn_graph, knn_graph.rs:337-360
  std::vector<std::pair<double, uint64_t>> nb;
  for (uint64_t i = 0; i < n; ++i) {
    nb.clear();
    for (uint64_t j = 0; j < n; ++j)
      if (j != i) nb.emplace_back(d[i * n + j], j);
    if (farthest)
      std::stable_sort(nb.begin(), nb.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    else
      std::stable_sort(nb.begin(), nb.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    const uint64_t take = std::min<uint64_t>(kk, nb.size());
    for (uint64_t t = 0; t < take; ++t) out->emplace_back(i, nb[t].second);
  }
}

// extract_tree_pairs_from_matrix, knn_graph.rs:243-286
int tree_pairs(swg_ctx* ctx, const double* d, uint64_t n, uint64_t near, uint64_t far, double rf, Pairs* out) {
  if (n < 2) return SWG_OK;
  Pairs all;
  if (near > 0) knn(d, n, near, false, &all);
  if (far > 0) knn(d, n, far, true, &all);
  if (rf > 0.0) {
    const int rc = random_pairs(ctx, n, rf, &all);
    if (rc != SWG_OK) return rc;
  }
  for (auto& p : all)
    if (p.first > p.second) std::swap(p.first, p.second);
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  out->insert(out->end(), all.begin(), all.end());
  return SWG_OK;
}

// select_pairs (no sketches, knn_graph.rs:400-489) and select_pairs_from_sketches (:498-560) over n haplotypes
int select(swg_ctx* ctx, const Strategy& st, const double* d, uint64_t n, Pairs* out) {
  switch (st.kind) {
    case Strategy::None:
    case Strategy::Wfmash:
      all_pairs(n, out);
      return SWG_OK;
    case Strategy::Random:
      return random_pairs(ctx, n, st.f, out);
    case Strategy::Auto:
      if (n <= 10) {
        all_pairs(n, out);
        return SWG_OK;
      }
      if (n <= 50) return select(ctx, Strategy{Strategy::Connectivity, 0.99}, d, n, out);
      return tree_pairs(ctx, d, n, 5, 2, 0.05, out);
    case Strategy::Connectivity: {
      const double nf = (double)n;
      const uint64_t target = (uint64_t)std::ceil(nf * std::log(nf) / 2.0 * (-std::log(st.f)));
      const uint64_t total = n * (n - 1) / 2;
      const double frac = std::fmin((double)target / (double)total, 1.0);  // f64::min: 0/0 = NaN -> 1.0
      const uint64_t kn = std::max<uint64_t>((uint64_t)std::ceil(frac * nf), 2);
      return tree_pairs(ctx, d, n, kn, 1, 0.01, out);
    }
    case Strategy::Tree:
      return tree_pairs(ctx, d, n, st.near, st.far, st.f, out);
  }
  return SWG_OK;
}

// extract_pansn_key(name, PanSnLevel::Haplotype), src/pansn.rs:58-86; None -> the whole name (:117)
inline bool ws(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }
std::string hap_key(const std::string& name) {
  size_t a = 0;
  while (a < name.size() && name[a] == '>') ++a;
  while (a < name.size() && ws((unsigned char)name[a])) ++a;
  size_t b = a;
  while (b < name.size() && !ws((unsigned char)name[b])) ++b;
  const std::string tok = name.substr(a, b - a);
  const std::string base = tok.substr(0, tok.find(':'));
  if (base.empty()) return name;
  const size_t h1 = base.find('#');
  const std::string sample = base.substr(0, h1);
  if (sample.empty()) return name;
  if (h1 == std::string::npos) return sample;
  const size_t h2 = base.find('#', h1 + 1);
  const std::string hap = base.substr(h1 + 1, h2 == std::string::npos ? std::string::npos : h2 - h1 - 1);
  return hap.empty() ? sample : sample + "#" + hap;
}

std::string sanitize(const std::string& s) {  // joblist.rs:102-113
  std::string o = s;
  for (auto& c : o)
    if (std::strchr("/\\#: \t*?\"<>|", c) && c) c = '_';
  return o;
}

std::string path_join(const std::string& dir, const std::string& name) {  // Path::join with a relative name
  if (dir.empty()) return name;
  return dir.back() == '/' ? dir + name : dir + "/" + name;
}

int host_error(swg_ctx* ctx, int code, const char* msg) { return swg_set_error(ctx, code, "%s", msg); }

double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

struct MergeSink {  // per-contig sketches gathered per haplotype (merge_sketches runs once every contig is in)
  std::vector<std::vector<uint64_t>>* hap;
  const std::vector<uint32_t>* hap_of;
};
void sink_emit(void* u, uint64_t i, const uint64_t* v, uint64_t n) {
  MergeSink* m = static_cast<MergeSink*>(u);
  auto& dst = (*m->hap)[(*m->hap_of)[i]];
  dst.insert(dst.end(), v, v + n);
}

}  // namespace

extern "C" int swg_mash_merge(const uint64_t* minimizers, const uint64_t* counts, uint64_t stride, const uint64_t* members,
                              uint64_t n_members, uint64_t s, uint64_t* out, uint64_t* out_count) {
  if (!out_count || (n_members && (!members || !counts || !minimizers)) || (s && !out)) return SWG_ERR_INVALID;
  std::vector<uint64_t> v;
  for (uint64_t m = 0; m < n_members; ++m) {
    const uint64_t c = counts[members[m]];
    if (c > stride) return SWG_ERR_INVALID;
    v.insert(v.end(), minimizers + members[m] * stride, minimizers + members[m] * stride + c);
  }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  if (v.size() > s) v.resize(s);
  if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(uint64_t));
  *out_count = v.size();
  return SWG_OK;
}

extern "C" int swg_select_pairs(swg_ctx* ctx, const char* strategy, const double* dist, uint64_t n, uint64_t** pairs_out,
                                uint64_t* n_pairs) {
  if (!strategy || !pairs_out || !n_pairs) return host_error(ctx, SWG_ERR_INVALID, "swg_select_pairs: NULL argument");
  *pairs_out = nullptr;
  *n_pairs = 0;
  Strategy st;
  if (!parse_strategy(strategy, &st)) return swg_set_error(ctx, SWG_ERR_INVALID, "invalid sparsification strategy '%s'", strategy);
  if (needs_sketches(st) && !dist && n > 1) return host_error(ctx, SWG_ERR_INVALID, "swg_select_pairs: this strategy needs the distance matrix");
  Pairs p;
  try {
    const int rc = select(ctx, st, dist, n, &p);
    if (rc != SWG_OK) return rc;
  } catch (...) {
    return host_error(ctx, SWG_ERR_OOM, "out of host memory selecting pairs");
  }
  uint64_t* o = static_cast<uint64_t*>(std::malloc(p.size() * 2 * sizeof(uint64_t) + 16));
  if (!o) return host_error(ctx, SWG_ERR_OOM, "out of host memory selecting pairs");
  for (size_t i = 0; i < p.size(); ++i) {
    o[2 * i] = p[i].first;
    o[2 * i + 1] = p[i].second;
  }
  *pairs_out = o;
  *n_pairs = p.size();
  return SWG_OK;
}

extern "C" int swg_joblist(swg_ctx* ctx, const char* const* paths, int n_paths, const char* strategy, int k, uint64_t s,
                           uint64_t threads, uint64_t min_aln_length, const char* output_dir, int io_threads, char** out_text,
                           uint64_t* out_len, double* timing_ms) {
  if (!out_text || !out_len || !strategy || n_paths < 1 || !paths) return host_error(ctx, SWG_ERR_INVALID, "swg_joblist: bad argument");
  *out_text = nullptr;
  *out_len = 0;
  Strategy st;
  if (!parse_strategy(strategy, &st)) return swg_set_error(ctx, SWG_ERR_INVALID, "invalid sparsification strategy '%s'", strategy);
  if (needs_sketches(st) && (k < 1 || k > 64 || s < 1 || s > 65536))
    return swg_set_error(ctx, SWG_ERR_UNSUPPORTED, "mash sketch: k must be in 1..64 and the sketch size in 1..65536 (got k=%d, s=%llu)", k,
                         (unsigned long long)s);
  const auto t_all = std::chrono::steady_clock::now();
  double t_read = 0, t_sketch = 0, t_merge = 0, t_dist = 0, t_select = 0;
  try {
    // ---- read: every file must be FASTA (main.rs:2713-2715)
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n_paths; ++i) {
      const std::string p = paths[i] ? paths[i] : "";
      const auto ends = [&](const char* suf) { return p.size() >= std::strlen(suf) && p.compare(p.size() - std::strlen(suf), std::string::npos, suf) == 0; };
      bool fasta = false;
      if (!ends(".agc") && !ends(".AGC") && !ends(".1aln")) {
        const char* data = nullptr;
        size_t len = 0;
        void* h = nullptr;
        const int rc = swg_host_text_load(p.c_str(), io_threads, &data, &len, &h);
        if (rc != SWG_OK) return swg_set_error(ctx, rc, "%s", swg_paf_last_error());
        fasta = swg_fasta_text_is_fasta(data, len);
        swg_host_text_release(h);
      }
      if (!fasta) return swg_set_error(ctx, SWG_ERR_INVALID, "--joblist requires FASTA inputs (got non-FASTA file %s)", p.c_str());
    }
    swg_fasta* fa = nullptr;
    int rc = swg_fasta_open(paths, n_paths, io_threads, &fa);
    if (rc != SWG_OK) return swg_set_error(ctx, rc, "%s", swg_fasta_last_error());
    struct Close {
      swg_fasta* f;
      ~Close() { swg_fasta_close(f); }
    } close_fa{fa};
    t_read = ms_since(t0);
    const uint64_t n = swg_fasta_num_records(fa);
    // ---- haplotypes (BTreeMap order) and the file of each (its first contig's)
    std::map<std::string, std::vector<uint64_t>> groups;
    std::vector<std::string> key(n);
    for (uint64_t i = 0; i < n; ++i) {
      key[i] = hap_key(swg_fasta_name(fa, i));
      groups[key[i]].push_back(i);
    }
    if (n == 0 || groups.size() == n)
      return host_error(ctx, SWG_ERR_UNSUPPORTED,
                        "--joblist: the input has no PanSN haplotype structure (SAMPLE#HAP#CONTIG names, several contigs per "
                        "haplotype); the per-file sweepga job list the reference emits for such input is not supported");
    const uint64_t nh = groups.size();
    std::vector<std::string> hap_name;
    std::vector<int> hap_file;
    std::vector<uint32_t> hap_of(n);
    for (auto& g : groups) {
      for (uint64_t c : g.second) hap_of[c] = (uint32_t)hap_name.size();
      hap_name.push_back(g.first);
      hap_file.push_back(swg_fasta_file_index(fa, g.second.front()));
    }
    // ---- haplotype sketches and distances (sketch-based strategies only, main.rs:894-925)
    std::vector<double> dist;
    if (needs_sketches(st)) {
      t0 = std::chrono::steady_clock::now();
      std::vector<std::vector<uint64_t>> hap(nh);
      MergeSink sink{&hap, &hap_of};
      rc = swg_mash_sketch_each(ctx, swg_fasta_bases(fa), swg_fasta_offsets(fa), n, k, s, sink_emit, &sink, nullptr);
      if (rc != SWG_OK) return rc;
      t_sketch = ms_since(t0);
      t0 = std::chrono::steady_clock::now();
      uint64_t stride = 1;
      for (auto& v : hap) {  // merge_sketches: sort, dedup, truncate
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        if (v.size() > s) v.resize(s);
        stride = std::max<uint64_t>(stride, v.size());
      }
      std::vector<uint64_t> flat(nh * stride, 0), cnt(nh);
      for (uint64_t h = 0; h < nh; ++h) {
        std::copy(hap[h].begin(), hap[h].end(), flat.begin() + h * stride);
        cnt[h] = hap[h].size();
      }
      t_merge = ms_since(t0);
      t0 = std::chrono::steady_clock::now();
      dist.assign(nh * nh, 0.0);
      rc = swg_mash_distances(ctx, flat.data(), cnt.data(), stride, nh, k, dist.data(), nullptr, nullptr);
      if (rc != SWG_OK) return rc;
      t_dist = ms_since(t0);
    }
    // ---- selection over haplotypes, then jobs: selected pairs + every self pair, in order
    t0 = std::chrono::steady_clock::now();
    Pairs sel;
    rc = select(ctx, st, dist.empty() ? nullptr : dist.data(), nh, &sel);
    if (rc != SWG_OK) return rc;
    for (uint64_t h = 0; h < nh; ++h) sel.emplace_back(h, h);
    for (auto& p : sel)
      if (p.first > p.second) std::swap(p.first, p.second);
    std::sort(sel.begin(), sel.end());
    sel.erase(std::unique(sel.begin(), sel.end()), sel.end());
    t_select = ms_since(t0);
    // ---- write_wfmash_pansn_commands, joblist.rs:124-145
    const std::string dir = output_dir ? output_dir : ".";
    std::string text;
    for (const auto& p : sel) {
      const std::string& tg = hap_name[p.first];
      const std::string& qy = hap_name[p.second];
      text += "wfmash -t " + std::to_string(threads);
      if (min_aln_length > 0) text += " -l " + std::to_string(min_aln_length);
      text += " -T " + tg + " -Q " + qy + " " + paths[hap_file[p.first]];
      if (hap_file[p.second] != hap_file[p.first] && std::strcmp(paths[hap_file[p.second]], paths[hap_file[p.first]]) != 0)
        text += std::string(" ") + paths[hap_file[p.second]];
      text += " > " + path_join(dir, sanitize(tg) + "_vs_" + sanitize(qy) + ".paf") + "\n";
    }
    char* o = text_copy(text);
    if (!o) return host_error(ctx, SWG_ERR_OOM, "out of host memory writing the job list");
    *out_text = o;
    *out_len = text.size();
  } catch (...) {
    return host_error(ctx, SWG_ERR_OOM, "out of host memory building the job list");
  }
  if (timing_ms) {
    timing_ms[0] = t_read;
    timing_ms[1] = t_sketch;
    timing_ms[2] = t_merge;
    timing_ms[3] = t_dist;
    timing_ms[4] = t_select;
    timing_ms[5] = ms_since(t_all);
  }
  return SWG_OK;
}
