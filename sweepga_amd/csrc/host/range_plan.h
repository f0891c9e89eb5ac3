// Host side of the ranged filter (csrc/swg_range.hip): a record set too large for one filter call -- 2^31 records or more, or
// a one-piece footprint beyond the context's device-memory limit -- is cut into ranges of whole genome pairs (first-two-'#'-
// parts rule, as csrc/host/shard_host.h), every range is filtered on its own, and the range-local chain numbers are made global
// again.  Genome pairs are independent units of the filter (every sweep segment, chain group, scaffold pair and rescue pair
// nests inside one), so the per-range results are those of the whole call.
//
//   pack     pairs in order of their first record, next-fit into ranges of at most R records; a pair larger than R forms a
//            range of its own (whether it fits the device is decided by running it); a pair of 2^31 records or more is refused
//   shifts   kept chains are numbered genome pair by genome pair in the order of the pairs' first retained records
//            (src/paf_filter.rs:517-521; shard_host.h merge() has the same rule): a pair's range-local numbers lo..hi become
//            offset + 1 .. offset + hi - lo + 1
//   largest  the largest range size whose estimated footprint fits a byte budget (the cost is monotone in the size)
//
// No HIP in this file: tests/native/range_plan_check.cpp exercises it on any machine.
#ifndef SWG_HOST_RANGE_PLAN_H
#define SWG_HOST_RANGE_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

namespace swg_range {

constexpr uint64_t MAX_RANGE = (uint64_t(1) << 31) - 1;  // one filter call holds fewer than 2^31 records

struct Range {
  std::vector<uint32_t> pairs;  // pair ids, in order of their first record
  uint64_t count = 0;           // records
  uint64_t lo = 0, hi = 0;      // smallest record index, largest + 1
  bool contiguous = false;      // the range is exactly the records [lo, hi) of the caller
  bool oversize = false;        // one pair of more than R records
};

enum PackResult { PACK_OK = 0, PACK_PAIR_TOO_LARGE = 1 };

// count[p] == 0: pair p does not occur.  first[p] / last[p]: its smallest / largest record index.  range_of[p] receives the
// range of pair p (UINT32_MAX for absent pairs).  On PACK_PAIR_TOO_LARGE *bad_pair is a pair of 2^31 records or more.
inline PackResult pack(uint32_t n_pairs, const uint64_t* count, const uint64_t* first, const uint64_t* last, uint64_t R,
                       std::vector<Range>* out, uint32_t* range_of, uint32_t* bad_pair) {
  out->clear();
  if (R < 1) R = 1;
  if (R > MAX_RANGE) R = MAX_RANGE;
  std::vector<uint32_t> order;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    range_of[p] = UINT32_MAX;
    if (!count[p]) continue;
    if (count[p] > MAX_RANGE) {
      *bad_pair = p;
      return PACK_PAIR_TOO_LARGE;
    }
    order.push_back(p);
  }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return first[a] != first[b] ? first[a] < first[b] : a < b; });
  auto close = [&]() {
    if (out->empty()) return;
    Range& g = out->back();
    g.contiguous = g.hi - g.lo == g.count;
  };
  for (uint32_t p : order) {
    const uint64_t c = count[p];
    if (c > R) {  // alone
      close();
      Range g;
      g.pairs.push_back(p);
      g.count = c;
      g.lo = first[p];
      g.hi = last[p] + 1;
      g.oversize = true;
      range_of[p] = (uint32_t)out->size();
      out->push_back(std::move(g));
      close();
      continue;
    }
    if (out->empty() || out->back().oversize || out->back().count + c > R) {
      close();
      out->emplace_back();
      out->back().lo = first[p];
      out->back().hi = last[p] + 1;
    }
    Range& g = out->back();
    g.pairs.push_back(p);
    g.count += c;
    g.lo = std::min(g.lo, first[p]);
    g.hi = std::max(g.hi, last[p] + 1);
    range_of[p] = (uint32_t)(out->size() - 1);
  }
  close();
  return PACK_OK;
}

// lo[p] / hi[p]: smallest / largest range-local kept chain number of pair p (hi == 0: none).  fret[p]: first record of the pair
// that passes the step-1 retain predicate.  shift[p] is added to every non-zero chain number of pair p.  Returns false when the
// global numbers reach 2^32 (chain_out is u32); *total receives the number of kept chains.
inline bool shifts(uint32_t n_pairs, const uint32_t* lo, const uint32_t* hi, const uint64_t* fret, int64_t* shift, uint64_t* total) {
  std::vector<uint32_t> with;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    shift[p] = 0;
    if (hi[p]) with.push_back(p);
  }
  std::stable_sort(with.begin(), with.end(), [&](uint32_t a, uint32_t b) { return fret[a] < fret[b]; });
  int64_t offset = 0;
  for (uint32_t p : with) {
    shift[p] = offset - ((int64_t)lo[p] - 1);
    offset += (int64_t)hi[p] - (int64_t)lo[p] + 1;
  }
  *total = (uint64_t)offset;
  return (uint64_t)offset <= 0xffffffffull;
}

// The largest m in [1, cap] with cost(m) <= budget (0 if not even one record fits).  cost must not decrease with m.
template <class F>
inline uint64_t largest(uint64_t cap, uint64_t budget, F&& cost) {
  if (cap < 1 || cost(1) > budget) return 0;
  uint64_t a = 1, b = cap;  // cost(a) <= budget
  while (a < b) {
    const uint64_t m = a + (b - a + 1) / 2;
    if (cost(m) <= budget) a = m; else b = m - 1;
  }
  return a;
}

}  // namespace swg_range
#endif
