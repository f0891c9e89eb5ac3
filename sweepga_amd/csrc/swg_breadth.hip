// Breadth: per ordered genome pair, the bases of each side that lie under at least one mapping -- the
// merged-interval coverage that alnstats' summed coverage is mistaken for -- for ALL records and, from the same launches, for
// the records a filter call KEPT (status != 0).  Only records whose two genomes differ count (alnstats' inter-genome rule).
//
// The unit is the filter's sweep segment: one sequence against one genome of the other side.  Per axis:
//
//   breadth_keys     key = segment << 32 | start, value = record index (bit 31: KEPT; n < 2^31 leaves it free, so the status
//                    byte is read once, in input order, and never gathered).  segment = sequence * G + genome of the other side
//                    while that fits 32 bits, else the slot of an open-addressing set over those products.  Records that do
//                    not count get the segment `sentinel` (one past the last id): they sort to the end and add nothing.
//   (sort)           swg_radix_sort_pairs over the 32 + bits(sentinel) key bits.
//   breadth_gather   tile of 1024 sorted records: end = end_column[record] (the one gather of the axis) written in sorted order,
//                    and the tile's maximum of P = segment << 32 | end, once over all records and once over the KEPT ones.
//                    Segments ascend along the sorted order, so the maximum of P over any prefix belongs to the LAST segment
//                    of the prefix: a plain running maximum of P is the segmented running maximum of the ends.  Also counts
//                    the segments (query axis), which bound the genome pairs that occur.
//   (scan)           swg_inclusive_max_scan_u64 over the tile maxima: the carry across work-groups, however far it reaches
//                    (one long interval over 10^6 short ones is 1000 tiles of carry).
//   breadth_union    the same tile again: carry-in = scanned maximum of the tile before, running maximum across the threads
//                    of the work-group (four consecutive records per thread, wavefront scan by shuffles, four wavefronts
//                    through LDS: running_max_before of swg_union_tiles.h), contribution = max(0, end - max(start, running
//                    maximum before)) with the maximum taken as 0 when it belongs to an earlier segment.  ALL and KEPT are two
//                    maxima in the same pass.  bases, union
//                    and the smallest record index go per genome pair through the run / LDS-table / global-table scheme of
//                    swg_pair_table.h: one atomic per (work-group, pair, quantity).
//   breadth_collect  the occupied pairs as lists (the host orders them by first record).
//
// Why two kernels around the library's scan and not one kernel with a decoupled look-back: a look-back makes work-groups wait
// for each other inside a launch, and a wait that is wrong hangs a device others share; this form has no wait, its cost is
// known -- the sorted keys, values and ends are read a second time, 16 bytes per record and axis -- and the scan it leans
// on runs over n / 1024 values.  tools/breadth_bench.py measures the split; DESIGN.md section 17 records what is known.
// Integer atomics only; no floating point.
#include <algorithm>
#include <cstdlib>
#include <new>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;   // the genome-pair table, the run and wavefront helpers, the host entry helpers
using namespace swg_union_tiles;  // the tile of the sorted order, its first pass and running maximum, the segment map, the front end
enum { D_BAD = 0, D_SEGMENTS, D_LISTED, D_LISTED_KEPT, D_TOTAL };
enum { Q_BASES = 0, Q_UNION, T_BASES, T_UNION, Q_COUNT };  // a listed entry's sums

using BreadthTable = PairTable<2 * Q_COUNT, true>;  // sums: [axis][bases ALL, union ALL, bases KEPT, union KEPT]
using BreadthList = PairList<2 * Q_COUNT, true>;   // entries: Q_BASES .. T_UNION and the first record of the set
// ---- keys --------------------------------------------------------------------------------------------------------------
template <int AXIS>
__global__ __launch_bounds__(TB) void breadth_keys_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                          const uint32_t* __restrict__ start, const uint8_t* __restrict__ status,
                                                          const uint32_t* __restrict__ seq_genome, uint32_t n_seq, SegMap M,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          unsigned long long* __restrict__ scalars) {
  segment_keys<AXIS>(n, q_id, t_id, start, status, seq_genome, n_seq, M, keys, vals, &scalars[D_BAD]);
}

// ---- one tile of the sorted order (load_tile, gather_tile, running_max_before: swg_union_tiles.h) ---------------------------------------------
__global__ __launch_bounds__(TB) void breadth_gather_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            const uint32_t* __restrict__ end_col, uint32_t sentinel,
                                                            uint32_t* __restrict__ ends, unsigned long long* __restrict__ tile_max,
                                                            uint64_t ntiles, unsigned long long* __restrict__ segments) {
  gather_tile<true>(n, keys, vals, end_col, sentinel, ends, tile_max, ntiles, segments);
}

template <int AXIS>
__global__ __launch_bounds__(TB) void breadth_union_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry,
                                                           uint64_t ntiles, uint32_t scanned, SegMap M, const uint32_t* __restrict__ seq_genome,
                                                           BreadthTable T) {
  __shared__ LdsTable<4, AXIS == 0> l_pairs;  // (first records: the query axis writes them, the target axis leaves them alone)
  __shared__ unsigned long long l_wave[2][WAVES];
  l_pairs.clear();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint64_t k[ITEMS];
  uint32_t v[ITEMS], e[ITEMS];
  load_tile(keys, vals, n, p0, k, v);
  load_ends(ends, n, p0, e);
  bool counted[ITEMS];
  unsigned long long t_max[2] = {0, 0};  // ALL, KEPT
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    counted[j] = p0 + j < n && (uint32_t)(k[j] >> 32) != M.sentinel;
    if (counted[j]) {
      const unsigned long long P = (k[j] & 0xffffffff00000000ull) | e[j];
      t_max[0] = max64(t_max[0], P);
      if (v[j] & KEPT_FLAG) t_max[1] = max64(t_max[1], P);
    }
  }
  unsigned long long r[2];
  running_max_before<2>(t_max, l_wave, carry, ntiles, scanned, r);  // (its barrier also: the LDS table is ready)
  unsigned long long r_all = r[0], r_kept = r[1];
  // contributions
  unsigned long long q[ITEMS][4];  // bases ALL, union ALL, bases KEPT, union KEPT
  uint32_t f_all[ITEMS], f_kept[ITEMS];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    q[j][0] = q[j][1] = q[j][2] = q[j][3] = 0;
    f_all[j] = f_kept[j] = NONE32;
    if (counted[j]) {
      const uint32_t seg = (uint32_t)(k[j] >> 32), start = (uint32_t)k[j], idx = v[j] & INDEX_MASK;
      const bool kept = (v[j] & KEPT_FLAG) != 0;
      const unsigned long long P = (k[j] & 0xffffffff00000000ull) | e[j];
      const uint32_t len = e[j] > start ? e[j] - start : 0u;
      const uint32_t m_all = (uint32_t)(r_all >> 32) == seg ? (uint32_t)r_all : 0u;
      const uint32_t lo_all = start > m_all ? start : m_all;
      q[j][0] = len;
      q[j][1] = e[j] > lo_all ? e[j] - lo_all : 0u;
      f_all[j] = idx;
      r_all = max64(r_all, P);
      if (kept) {
        const uint32_t m_kept = (uint32_t)(r_kept >> 32) == seg ? (uint32_t)r_kept : 0u;
        const uint32_t lo_kept = start > m_kept ? start : m_kept;
        q[j][2] = len;
        q[j][3] = e[j] > lo_kept ? e[j] - lo_kept : 0u;
        f_kept[j] = idx;
        r_kept = max64(r_kept, P);
      }
    }
  }
  // a thread's records of one segment: summed towards the first of them
  bool head[ITEMS];
#pragma unroll
  for (int j = ITEMS - 1; j >= 1; --j) {
    head[j] = counted[j];
    if (counted[j] && counted[j - 1] && (k[j] >> 32) == (k[j - 1] >> 32)) {
#pragma unroll
      for (int c = 0; c < 4; ++c) q[j - 1][c] += q[j][c];
      f_all[j - 1] = f_all[j - 1] < f_all[j] ? f_all[j - 1] : f_all[j];
      f_kept[j - 1] = f_kept[j - 1] < f_kept[j] ? f_kept[j - 1] : f_kept[j];
      head[j] = false;
    }
  }
  head[0] = counted[0];
  // round j: what the lanes hold at place j, runs of one genome pair along the lanes summed towards the run's first lane
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (__ballot(head[j]) == 0) continue;  // wavefront-uniform (rounds 1..3: only where a segment starts inside a thread)
    unsigned long long key = EMPTY;
    if (head[j]) {
      uint32_t seq, other;
      segment_of(M, (uint32_t)(k[j] >> 32), &seq, &other);
      const uint32_t mine = seq_genome[seq];
      key = AXIS ? (unsigned long long)other * M.G + mine : (unsigned long long)mine * M.G + other;
    }
    const unsigned long long before = __shfl_up(key, 1);
    const bool first_lane = lane == 0 || key != before;
    const int end = run_end(__ballot(first_lane), lane);
    run_sum(q[j], lane, end);
    uint32_t fa = f_all[j], fk = f_kept[j];
    if (AXIS == 0) {
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t a = __shfl_down(fa, d), b = __shfl_down(fk, d);
        if (lane + d < end) fa = fa < a ? fa : a, fk = fk < b ? fk : b;
      }
    }
    if (first_lane && key != EMPTY) {
      if (!l_pairs.add(key, q[j], fa, fk))
        table_add<4, AXIS == 0>(T, key, q[j], 4 * AXIS, fa, fk);  // more pairs in this tile than the LDS table takes
    }
  }
  __syncthreads();
  l_pairs.flush(T, 4 * AXIS);
}

// ---- the occupied genome pairs as lists ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void breadth_collect_kernel(BreadthTable T, BreadthList L) { list_slots(T, L); }

// inside an arena frame
int breadth_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const SegCols& d, swg_breadth_result* all, swg_breadth_result* kept) {
  hipStream_t st = ctx->stream;
  const bool force_hash = segmap_forced();  // test knob: the hashed segment set and pair table at any size
  const uint64_t ntiles = (n + TILE - 1) / TILE;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  uint64_t* keys = swg_alloc<uint64_t>(ctx, n);
  uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n);
  uint32_t* vals = swg_alloc<uint32_t>(ctx, n);
  uint32_t* vals_alt = swg_alloc<uint32_t>(ctx, n);
  uint32_t* ends = swg_alloc<uint32_t>(ctx, n);
  unsigned long long* tile_max = swg_alloc<unsigned long long>(ctx, 2 * ntiles);
  SegMap M;
  segmap_alloc(ctx, n, n_seq, G, force_hash, &M);  // (swg_union_tiles.h)
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  const int end_bit = 32 + swg_bits_for(M.sentinel);
  const unsigned grid_n = (unsigned)((n + TB - 1) / TB), grid_t = (unsigned)ntiles;
  const uint32_t scanned = d.status ? 3u : 1u;  // (no status: nothing is KEPT, and the KEPT maxima are not scanned)
  BreadthTable T{};
  BreadthList L{};
  for (int axis = 0; axis < 2; ++axis) {
    if (M.set_keys) SWG_HIP(ctx, hipMemsetAsync(M.set_keys, 0xff, ((size_t)M.set_mask + 1) * sizeof(unsigned long long), st));
    if (axis == 0)
      SWG_LAUNCH(ctx, "breadth_keys", breadth_keys_kernel<0><<<grid_n, TB, 0, st>>>(n, d.q_id, d.t_id, d.start[0], d.status, d.seq_genome,
                                                                                     n_seq, M, keys, vals, scalars));
    else
      SWG_LAUNCH(ctx, "breadth_keys", breadth_keys_kernel<1><<<grid_n, TB, 0, st>>>(n, d.q_id, d.t_id, d.start[1], d.status, d.seq_genome,
                                                                                     n_seq, M, keys, vals, scalars));
    SWG_KERNEL_CHECK(ctx);
    {  // (the profiler sees the axis' sort as one entry too: with swg_profile_select, the sort of this call's pairs on its own)
      swg_prof_scope sort_scope(ctx, axis == 0 ? "breadth_sort_q" : "breadth_sort_t");
      SWG_TRY(swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, n, 0, end_bit));
    }
    SWG_LAUNCH(ctx, "breadth_gather", breadth_gather_kernel<<<grid_t, TB, 0, st>>>(n, keys, vals, d.end[axis], M.sentinel, ends, tile_max, ntiles,
                                                                                     axis == 0 ? scalars + D_SEGMENTS : nullptr));
    SWG_KERNEL_CHECK(ctx);
    if (axis == 0) {
      uint64_t h[2];
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 2));
      if (h[D_BAD]) return swg_set_error(ctx, SWG_ERR_INVALID, "breadth: a sequence id >= n_seq or a genome id >= n_genome");
      // genome pairs that occur <= segments of the query axis (every pair has one)
      const uint64_t g2 = (uint64_t)G * G;
      SWG_TRY(table_create(ctx, G, g2 < h[D_SEGMENTS] ? g2 : h[D_SEGMENTS], force_hash, d.status != nullptr, scalars + D_LISTED, &T, &L));
    }
    SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max), reinterpret_cast<uint64_t*>(tile_max), ntiles));
    if (d.status)
      SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max + ntiles), reinterpret_cast<uint64_t*>(tile_max + ntiles), ntiles));
    if (axis == 0)
      SWG_LAUNCH(ctx, "breadth_union", breadth_union_kernel<0><<<grid_t, TB, 0, st>>>(n, keys, vals, ends, tile_max, ntiles, scanned, M,
                                                                                       d.seq_genome, T));
    else
      SWG_LAUNCH(ctx, "breadth_union", breadth_union_kernel<1><<<grid_t, TB, 0, st>>>(n, keys, vals, ends, tile_max, ntiles, scanned, M,
                                                                                       d.seq_genome, T));
    SWG_KERNEL_CHECK(ctx);
  }
  SWG_LAUNCH(ctx, "breadth_collect", breadth_collect_kernel<<<(unsigned)((T.slots + TB - 1) / TB), TB, 0, st>>>(T, L));
  SWG_KERNEL_CHECK(ctx);
  uint64_t h[D_TOTAL];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  std::vector<BreadthList::Entry> list[2];
  SWG_TRY(list_fetch(ctx, "breadth", L, h + D_LISTED, list));
  swg_breadth_result* res[2] = {all, d.status ? kept : nullptr};
  for (int s = 0; s < 2; ++s) {
    if (!res[s]) continue;
    res[s]->pairs.resize(list[s].size());
    for (size_t k = 0; k < list[s].size(); ++k) {
      const BreadthList::Entry& o = list[s][k];
      res[s]->pairs[k] = swg_breadth_pair{(uint32_t)(o.key / G), (uint32_t)(o.key % G), o.v[Q_BASES], o.v[T_BASES], o.v[Q_UNION], o.v[T_UNION], o.first};
    }
  }
  return SWG_OK;
}

void hand_over(const swg_breadth_result& r, swg_breadth_counts* c) {
  if (!c) return;
  c->n_pairs = r.pairs.size();
  if (c->pairs && c->n_pairs <= c->pair_capacity) std::copy(r.pairs.begin(), r.pairs.end(), c->pairs);
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                swg_breadth_counts* all, swg_breadth_counts* kept) {
  if (!ctx) return SWG_ERR_INVALID;
  try {
    swg_breadth_result ra, rk;
    SWG_TRY(swg_breadth_run(ctx, rec, on_device, seq_genome, n_genome, status, all ? &ra : nullptr, kept && status ? &rk : nullptr));
    hand_over(ra, all);
    if (status) hand_over(rk, kept);
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

int swg_breadth_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome,
                    const uint8_t* status, swg_breadth_result* all, swg_breadth_result* kept) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec) return swg_set_error(ctx, SWG_ERR_INVALID, "breadth: NULL records");
  const uint64_t n = rec->n;
  if (all) all->pairs.clear();
  if (kept) kept->pairs.clear();
  if (n == 0) return SWG_OK;
  SWG_TRY(seg_check_args(ctx, "breadth", ARG_COLUMNS | ARG_COUNTS | ARG_LIMIT, rec, seq_genome, n_genome, 31));
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 64 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    SegCols d;
    SWG_TRY(seg_stage(ctx, rec, on_device, seq_genome, status, &d));
    return breadth_device(ctx, n, rec->n_seq, n_genome, d, all, kept);
  });
}

extern "C" int swg_breadth_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                   const uint8_t* status, swg_breadth_counts* all, swg_breadth_counts* kept) {
  return records_abi(ctx, rec, false, seq_genome, n_genome, status, all, kept);
}

extern "C" int swg_breadth_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                          const uint8_t* status, swg_breadth_counts* all, swg_breadth_counts* kept) {
  return records_abi(ctx, rec, true, seq_genome, n_genome, status, all, kept);
}

// The breadth report of an open PAF: records and genome map from the handle, the integers from the device, the genome sizes as
// swg_paf_alnstats derives them -- the last line per sequence and set comes from the alnstats kernels, its length from the
// handle's text (host/paf_io.cpp) -- and the text from host/alnstats.cpp.  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_breadth(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, int detailed, char** out_text, uint64_t* out_len) {
  if (out_text) *out_text = nullptr;
  if (out_len) *out_len = 0;
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_breadth: NULL argument");
  const uint64_t n = swg_paf_records(p)->n;
  if (n && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_breadth: NULL context");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED, "swg_paf_breadth: the file has a value >= 2^32, its columns are rebased: breadth of 64-bit columns is not supported");
  try {
    swg_records rec;
    std::vector<uint32_t> col10;
    const uint32_t* seq_genome = nullptr;
    SWG_TRY(swg_paf_stats_prepare(p, &rec, &col10, &seq_genome));
    swg_alnstats_result stats[2];
    swg_breadth_result res[2];
    if (n) {
      int rc = swg_alnstats_run(ctx, &rec, false, seq_genome, rec.n_genome_last, status, &stats[0], status ? &stats[1] : nullptr);
      if (rc == SWG_OK) rc = swg_breadth_run(ctx, &rec, false, seq_genome, rec.n_genome_last, status, &res[0], status ? &res[1] : nullptr);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    }
    std::vector<std::string> gname;
    std::vector<uint64_t> gsize[2];
    swg_paf_stats_genome_names(p, &gname);
    for (int k = 0; k < (status ? 2 : 1); ++k) SWG_TRY(swg_paf_stats_genome_sizes(p, stats[k], &gsize[k]));
    return swg_breadth_report(gname, res, gsize, status ? 2 : 1, detailed != 0, out_text, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
