// Tree sparsification of a PAF before the filter: `--sparsify tree:<near>[:<far>[:<random>]]` (or `knn:`), which the
// reference applies to the input file before PafFilter::filter_paf (src/main.rs:3640-3688, src/tree_filter.rs:205-285).
//
//   1. every line that is neither empty nor '#'-led and has >= 11 fields is an alignment: genome = first two '#' parts of
//      the name + '#' (the whole name without '#'), matches / block length = columns 10 / 11 (0 / 1 when unparsable);
//   2. per unordered pair of different genomes: identity = sum(matches) / sum(block length)   (src/tree_filter.rs:39-75);
//   3. every genome keeps its k_nearest best and k_farthest worst neighbours by that identity (:79-135), plus every pair
//      whose DefaultHasher (SipHash-1-3, zero keys) value over the two prefixes is <= random_fraction * 2^64 (:137-156);
//   4. the lines of the selected pairs survive, in input order, newline-normalised (:172-200, 277-282).
// Equal identities: the reference sorts a HashMap's iteration order (arbitrary between runs); here ties fall to the
// neighbour's prefix in ascending byte order, i.e. one of the orders the reference can produce.
// Steps 2-3 are swg_tree_select below: ONE implementation, over (pair sums, genome prefixes), shared by this text route and by
// the record routes (swg_sparsify.hip), whose sums come from the device.  The text route is the tool for PAF text and the
// fall-back of swg_paf_tree_select for a handle whose columns are not what step 1 reads.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../../include/sweepga_gpu.h"
#include "host_internal.h"

namespace {

std::string genome_of(std::string_view name) {  // src/tree_filter.rs:15-24
  const size_t a = name.find('#');
  if (a == std::string_view::npos) return std::string(name);
  const size_t b = name.find('#', a + 1);
  std::string g(name.substr(0, b == std::string_view::npos ? name.size() : b));
  g.push_back('#');
  return g;
}

uint64_t number_or(std::string_view f, uint64_t fallback) {  // str::parse::<u64>().unwrap_or(fallback)
  size_t i = (!f.empty() && f[0] == '+') ? 1 : 0;
  if (i >= f.size()) return fallback;
  unsigned __int128 v = 0;
  for (; i < f.size(); ++i) {
    if (f[i] < '0' || f[i] > '9') return fallback;
    v = v * 10 + (unsigned)(f[i] - '0');
    if (v > UINT64_MAX) return fallback;
  }
  return (uint64_t)v;
}

// SipHash-1-3 with zero keys over one byte string (what DefaultHasher::new() computes for the concatenated writes)
uint64_t sip13(const std::string& bytes) {
  uint64_t v[4] = {0x736f6d6570736575ull, 0x646f72616e646f6dull, 0x6c7967656e657261ull, 0x7465646279746573ull};
  auto rot = [](uint64_t x, int k) { return (x << k) | (x >> (64 - k)); };
  auto mix = [&]() {
    v[0] += v[1]; v[2] += v[3];
    v[1] = rot(v[1], 13) ^ v[0]; v[3] = rot(v[3], 16) ^ v[2];
    v[0] = rot(v[0], 32);
    v[2] += v[1]; v[0] += v[3];
    v[1] = rot(v[1], 17) ^ v[2]; v[3] = rot(v[3], 21) ^ v[0];
    v[2] = rot(v[2], 32);
  };
  const size_t n = bytes.size(), full = n / 8 * 8;
  for (size_t i = 0; i < full; i += 8) {
    uint64_t m;
    std::memcpy(&m, bytes.data() + i, 8);  // little-endian host
    v[3] ^= m;
    mix();
    v[0] ^= m;
  }
  uint64_t last = (uint64_t)(n & 0xff) << 56;
  for (size_t i = full; i < n; ++i) last |= (uint64_t)(unsigned char)bytes[i] << (8 * (i - full));
  v[3] ^= last;
  mix();
  v[0] ^= last;
  v[2] ^= 0xff;
  mix();
  mix();
  mix();
  return v[0] ^ v[1] ^ v[2] ^ v[3];
}

}  // namespace


// Steps 2-3 over pair sums: selected[k] = 1 when pairs[k] survives.  Every pair has prefix[a] < prefix[b] (the reference's
// canonical order) and occurs once.
void swg_tree_select(const std::vector<std::string>& prefix, const std::vector<swg_tree_pair>& pairs, uint64_t k_nearest,
                     uint64_t k_farthest, double random_fraction, std::vector<uint8_t>* selected) {
  selected->assign(pairs.size(), 0);
  struct Nb {
    uint32_t other, pair;
    double identity;
  };
  std::vector<std::vector<Nb>> nbs(prefix.size());
  for (size_t k = 0; k < pairs.size(); ++k) {
    const swg_tree_pair& p = pairs[k];
    const double id = p.block > 0.0 ? p.matches / p.block : 0.0;
    nbs[p.a].push_back({p.b, (uint32_t)k, id});
    nbs[p.b].push_back({p.a, (uint32_t)k, id});
  }
  for (std::vector<Nb>& v : nbs) {
    if (v.empty()) continue;
    // identity descending; ties: neighbour prefix ascending (stable order of the reference's arbitrary one)
    std::sort(v.begin(), v.end(), [&](const Nb& x, const Nb& y) {
      if (x.identity != y.identity) return x.identity > y.identity;
      return prefix[x.other] < prefix[y.other];
    });
    for (size_t k = 0; k < v.size() && k < k_nearest; ++k) (*selected)[v[k].pair] = 1;
    for (size_t k = 0; k < v.size() && k < k_farthest; ++k) (*selected)[v[v.size() - 1 - k].pair] = 1;  // the reversed list
  }
  if (random_fraction > 0.0) {
    const double scaled = random_fraction * 18446744073709551616.0;  // u64::MAX as f64
    const uint64_t threshold = scaled >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)scaled;  // `as u64` saturates
    std::string buf;
    for (size_t k = 0; k < pairs.size(); ++k) {
      buf.assign(prefix[pairs[k].a]);
      buf.push_back((char)0xff);
      buf.append(prefix[pairs[k].b]);
      buf.push_back((char)0xff);
      if (sip13(buf) <= threshold) (*selected)[k] = 1;
    }
  }
}

namespace {

struct Line {
  uint64_t off;
  uint32_t len;
  uint8_t keep;
};

// steps 1-3 over PAF text: the alignment lines with their verdicts
int scan_text(const char* text, uint64_t len, uint64_t k_nearest, uint64_t k_farthest, double random_fraction, std::vector<Line>* out) {
  struct Aln {
    uint32_t gq, gt;
  };
  std::vector<Line>& alns = *out;
  std::vector<Aln> ag;
  std::vector<std::string> genomes;  // id -> prefix
  std::unordered_map<std::string, uint32_t> gid;
  std::unordered_map<std::string_view, uint32_t> name_gid;  // sequence name -> genome id (names repeat, prefixes are built once)
  auto genome_id = [&](std::string_view name) {
    auto it = name_gid.find(name);
    if (it != name_gid.end()) return it->second;
    std::string g = genome_of(name);
    auto jt = gid.find(g);
    uint32_t id;
    if (jt == gid.end()) {
      id = (uint32_t)genomes.size();
      gid.emplace(g, id);
      genomes.push_back(std::move(g));
    } else {
      id = jt->second;
    }
    name_gid.emplace(name, id);
    return id;
  };
  std::unordered_map<uint64_t, uint32_t> pair_of;  // key = smaller-prefix genome id << 32 | the other one -> index in `pairs`
  std::vector<swg_tree_pair> pairs;
  auto pair_key = [&](uint32_t a, uint32_t b) {
    if (genomes[b] < genomes[a]) std::swap(a, b);
    return ((uint64_t)a << 32) | b;
  };
  for (uint64_t pos = 0; pos < len;) {
    const char* nl = static_cast<const char*>(std::memchr(text + pos, '\n', len - pos));
    const uint64_t end = nl ? (uint64_t)(nl - text) : len;
    uint64_t ll = end - pos;
    if (nl && ll && text[end - 1] == '\r') --ll;  // BufRead::lines strips "\n" and "\r\n"
    const std::string_view line(text + pos, ll);
    const uint64_t here = pos;
    pos = end + 1;
    if (line.empty() || line[0] == '#') continue;
    std::string_view f[11];
    size_t s0 = 0;
    int nf = 0;
    while (nf < 11) {
      const size_t t = line.find('\t', s0);
      f[nf++] = line.substr(s0, t == std::string_view::npos ? std::string_view::npos : t - s0);
      if (t == std::string_view::npos) break;
      s0 = t + 1;
    }
    if (nf < 11) continue;
    if (ll > 0xffffffffull) return SWG_ERR_RANGE;
    const Aln a{genome_id(f[0]), genome_id(f[5])};
    alns.push_back(Line{here, (uint32_t)ll, 0});
    ag.push_back(a);
    if (a.gq == a.gt) continue;
    const uint64_t key = pair_key(a.gq, a.gt);
    auto it = pair_of.find(key);
    if (it == pair_of.end()) {
      it = pair_of.emplace(key, (uint32_t)pairs.size()).first;
      pairs.push_back(swg_tree_pair{(uint32_t)(key >> 32), (uint32_t)key, 0.0, 0.0});
    }
    pairs[it->second].matches += (double)number_or(f[9], 0);
    pairs[it->second].block += (double)number_or(f[10], 1);
  }
  std::vector<uint8_t> selected;
  swg_tree_select(genomes, pairs, k_nearest, k_farthest, random_fraction, &selected);
  for (size_t i = 0; i < alns.size(); ++i)
    alns[i].keep = ag[i].gq != ag[i].gt && selected[pair_of.find(pair_key(ag[i].gq, ag[i].gt))->second];
  return SWG_OK;
}

}  // namespace

extern "C" int swg_paf_tree_filter(const char* text, uint64_t len, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                                   char** out_text, uint64_t* out_len) {
  if (!out_text || !out_len || (len && !text)) return SWG_ERR_INVALID;
  *out_text = nullptr;
  *out_len = 0;
  try {
    std::vector<Line> alns;
    const int rc = scan_text(text, len, k_nearest, k_farthest, random_fraction, &alns);
    if (rc != SWG_OK) return rc;
    uint64_t total = 0;
    for (const Line& a : alns)
      if (a.keep) total += (uint64_t)a.len + 1;
    char* out = static_cast<char*>(std::malloc(total ? total : 1));
    if (!out) return SWG_ERR_OOM;
    uint64_t o = 0;
    for (const Line& a : alns)
      if (a.keep) {
        std::memcpy(out + o, text + a.off, a.len);
        o += a.len;
        out[o++] = '\n';
      }
    *out_text = out;
    *out_len = o;
  } catch (const std::bad_alloc&) {
    return SWG_ERR_OOM;
  }
  return SWG_OK;
}

// The text route's verdicts as a mask over a handle's records (rec_off[n]: ascending byte offsets of the records' lines in the
// same text): a record is kept when its line is one of the lines swg_paf_tree_filter would write.
int swg_tree_text_mask(const char* text, uint64_t len, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                       const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t* n_kept) {
  try {
    std::vector<Line> alns;
    const int rc = scan_text(text, len, k_nearest, k_farthest, random_fraction, &alns);
    if (rc != SWG_OK) return rc;
    uint64_t kept = 0;
    size_t j = 0;
    for (uint64_t i = 0; i < n; ++i) {
      while (j < alns.size() && alns[j].off < rec_off[i]) ++j;
      keep[i] = j < alns.size() && alns[j].off == rec_off[i] && alns[j].keep;
      kept += keep[i];
    }
    if (n_kept) *n_kept = kept;
  } catch (const std::bad_alloc&) {
    return SWG_ERR_OOM;
  }
  return SWG_OK;
}

extern "C" int swg_tree_select_pairs(uint32_t n_genome, const char* const* genome_prefix, uint64_t n_pairs, const uint32_t* pair_a,
                                     const uint32_t* pair_b, const uint64_t* sum_matches, const uint64_t* sum_block_len,
                                     uint64_t k_nearest, uint64_t k_farthest, double random_fraction, uint8_t* selected) {
  if ((n_genome && !genome_prefix) || (n_pairs && (!pair_a || !pair_b || !sum_matches || !sum_block_len || !selected))) return SWG_ERR_INVALID;
  try {
    std::vector<std::string> prefix(n_genome);
    for (uint32_t g = 0; g < n_genome; ++g) {
      if (!genome_prefix[g]) return SWG_ERR_INVALID;
      prefix[g] = genome_prefix[g];
    }
    std::vector<swg_tree_pair> pairs(n_pairs);
    std::unordered_set<uint64_t> seen;
    for (uint64_t k = 0; k < n_pairs; ++k) {
      uint32_t a = pair_a[k], b = pair_b[k];
      if (a >= n_genome || b >= n_genome || prefix[a] == prefix[b]) return SWG_ERR_INVALID;
      if (sum_matches[k] >= SWG_TREE_SUM_LIMIT || sum_block_len[k] >= SWG_TREE_SUM_LIMIT) return SWG_ERR_RANGE;
      if (prefix[b] < prefix[a]) std::swap(a, b);
      if (!seen.insert(((uint64_t)a << 32) | b).second) return SWG_ERR_INVALID;  // a pair listed twice
      pairs[k] = swg_tree_pair{a, b, (double)sum_matches[k], (double)sum_block_len[k]};
    }
    std::vector<uint8_t> sel;
    swg_tree_select(prefix, pairs, k_nearest, k_farthest, random_fraction, &sel);
    std::copy(sel.begin(), sel.end(), selected);
  } catch (const std::bad_alloc&) {
    return SWG_ERR_OOM;
  }
  return SWG_OK;
}

extern "C" void swg_free(void* p) { std::free(p); }
