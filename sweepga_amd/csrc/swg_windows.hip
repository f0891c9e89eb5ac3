// Windows: per fixed window of W bases along every sequence that carries a record, how many records touch
// it (n), how deep the pile is (depth), how much of it is covered at all (covered, the union) and how many matches fall into it
// (matches), for ALL records and for the records a filter call KEPT, from one call.  include/sweepga_gpu.h states the definitions.
// On axis 0 the sequence s is q_id and the other sequence o is t_id; on axis 1 the columns swap (Cols holds them by role).
//
// A record is accounted for in a constant number of updates, whatever its length.  With k0 = a / W and k1 = (b - 1) / W it adds
//   at k0        1 to `starts`, and to the edge accumulators its overlap with window k0 and the matches that go with it;
//   at k1        1 to `ends`, and for k1 > k0 its overlap with window k1 and those matches;
//   k1 > k0 + 1  the windows k0 + 1 .. k1 - 1 lie inside it: +1 / -1 at k0 + 1 / k1 of a "full" difference array and +c / -c
//                (c = floor(W m / (b - a))) at the same slots of a matches-difference array.
// Prefix sums over the table fill in the rest: n = starts up to and including the window minus ends before it, depth = edge +
// W * full, matches = edge + the matches prefix.  The table is dense over the listed sequences (base[s] = the windows of the
// listed sequences before s, T in all) and the prefixes run over all of it without segments: a record starts and ends, and a
// difference opens and closes, inside its own sequence, so everything an earlier sequence added has cancelled where the next one
// begins.  The 64-bit differences wrap modulo 2^64; every true prefix is below 2^63, so the prefix is exact.
//
//   windows_keys        one pass over the records: the id checks, who takes part (ALL, KEPT), the smallest record that ends beyond
//                       its sequence, the listed flags, and the sort key = s << 32 | a with value = record | KEPT_FLAG; the others
//                       get the sentinel n_seq.
//   windows_counts      K_s of every listed sequence, 0 for the others; swg_inclusive_sum_scan_u64 gives base and T.  The host
//                       refuses T >= 2^31 here, before anything of that size is allocated.
//   (sort)              swg_radix_sort_pairs over 32 + bits(n_seq) bits, then the walk of swg_union_tiles.h with the SEQUENCE as
//                       the unit: windows_gather (ends in sorted order, tile maxima), swg_inclusive_max_scan_u64 over the maxima,
//   windows_walk        and the second pass, which does all the accounting in the sorted order.  Union: what a record adds to the
//                       union of its set is [max(a, running maximum before), b); these pieces are disjoint and tile the union, so
//                       they feed a covered edge accumulator and a covered-difference array exactly as records feed depth.  Depth:
//                       neighbours in the sorted order start in the same window more often than not (a pile 60 deep puts 60
//                       neighbours on one window), so what the lanes of a wavefront add at one slot is summed along the lanes
//                       first (runs of one slot, run_end / run_sum of swg_pair_table.h) and the run's first lane issues the
//                       atomic: DESIGN.md section 13 (3).  The k1 side folds the same way (ends are not sorted, but neighbours
//                       mostly end in the same window too; any split into runs is correct).  Interior differences are rare
//                       (records longer than W) and go one by one.
//   (scans)             swg_inclusive_sum_scan_u64 over the five count / difference arrays of every set.
//   windows_rows        one lane per window: its sequence by binary search over the scanned counts, then the sums above.  With
//                       the summary it leaves empty / covered / depth / matches of the window in arrays that this lane alone has
//                       read (edge_depth, dcov, dfull, dm),
//   (scans)             which are summed, and
//   windows_seqs        one lane per listed sequence takes the differences of those sums -- and of the starts' prefix: the
//                       records that take part -- at its two ends.
//
// No kernel waits for another work-group.  Integer atomics only (64-bit adds, 32-bit adds for covered edges, one 64-bit minimum):
// all updates commute, nothing depends on record order or grid shape.
//
// Device memory, from the context's arena: 28 bytes per record (two 8-byte key and two 4-byte value buffers, the ends) plus the
// radix sort's histograms and 16 bytes per tile of 1,024 records; 9 bytes per sequence (listed flag, count prefix) and 4 per listed
// sequence; 120 bytes per window (per set five 8-byte count / difference arrays, two 8-byte and one 4-byte edge accumulator) plus
// 64 for its row, and 80 per listed sequence with the summary.  The host seam stages the two ids, the axis' two coordinates, the
// weight and the status: 21 bytes per record more, and 8 per sequence.
#include <new>
#include <string>
#include <vector>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "host/host_internal.h"

namespace {

using namespace swg_union_tiles;  // the tile of the sorted order, its first pass and running maximum, rows_hand_over
using swg_pair_table::EMPTY;
using swg_pair_table::grid_for;
using swg_pair_table::NONE32;
using swg_pair_table::reserve_first;
using swg_pair_table::run_end;
using swg_pair_table::run_sum;

enum { D_BAD_ID = 0, D_BAD_END, D_COUNT, D_TOTAL };
constexpr uint64_t MAX_WINDOWS = uint64_t(1) << 31;
static_assert(sizeof(swg_window_row) == 64 && sizeof(swg_window_seq) == 80 && sizeof(swg_windows_request) == 80, "include/sweepga_gpu.h states these sizes");

struct Cols {  // by role: s = the sequence the windows lie on, o = the other one; [a, b) on s, m = the record's matches
  const uint32_t *s_id, *o_id, *a, *b, *m, *seq_genome, *seq_len;
  const uint8_t* status;  // nullptr = there is no KEPT set
};

struct Acc {  // the window table, per set; T entries each
  unsigned long long *starts[2], *ends[2];               // records whose first / last window this is
  unsigned long long *dfull[2], *dm[2], *dcov[2];        // differences: records that fill the window, their matches, union pieces that fill it
  unsigned long long *edge_depth[2], *edge_matches[2];   // what the first and last windows of the records add
  uint32_t* edge_cov[2];                                 // what the first and last windows of the union's pieces add (disjoint pieces: <= W)
};

// ---- ids, who takes part, the listed sequences, the keys -------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void windows_keys_kernel(uint64_t n, Cols c, uint32_t n_seq, uint32_t G, uint32_t other, uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ vals, uint8_t* __restrict__ listed, unsigned long long* __restrict__ scalars) {
  for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TB) {
    const uint32_t s = c.s_id[i], o = c.o_id[i], a = c.a[i], b = c.b[i];
    const uint32_t gs = s < n_seq ? c.seq_genome[s] : NONE32, go = o < n_seq ? c.seq_genome[o] : NONE32;  // (no gather before the id is known)
    const bool wrong = gs >= G || go >= G;
    const bool takes = !wrong && gs != go && a < b && (other == SWG_WINDOWS_ANY || go == other);
    const bool kept = takes && c.status && c.status[i] != 0;
    if (wrong) atomicOr(&scalars[D_BAD_ID], 1ull);
    if (takes && b > c.seq_len[s]) atomicMin(&scalars[D_BAD_END], (unsigned long long)i);
    keys[i] = takes ? ((uint64_t)s << 32) | a : (uint64_t)n_seq << 32;
    vals[i] = (uint32_t)i | (kept ? KEPT_FLAG : 0u);
    if (takes && !listed[s]) listed[s] = 1;  // (every writer stores the same byte; the test spares the store, not the answer)
  }
}

__global__ __launch_bounds__(TB) void windows_counts_kernel(uint32_t n_seq, const uint8_t* __restrict__ listed, const uint32_t* __restrict__ seq_len, uint32_t W,
                                                            unsigned long long* __restrict__ count) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (s < n_seq) count[s] = listed[s] ? ((unsigned long long)seq_len[s] + W - 1) / W : 0ull;
}

// incl: the inclusive sums of the counts.  The first window of sequence s in the table
__device__ __forceinline__ unsigned long long base_of(const unsigned long long* __restrict__ incl, uint32_t s) { return s ? incl[s - 1] : 0ull; }

// ---- the walk over the sorted order: union, and the accounting of every record ----------------------------------------------------
__global__ __launch_bounds__(TB) void windows_gather_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            const uint32_t* __restrict__ end_col, uint32_t sentinel, uint32_t* __restrict__ ends,
                                                            unsigned long long* __restrict__ tile_max, uint64_t ntiles) {
  gather_tile<true>(n, keys, vals, end_col, sentinel, ends, tile_max, ntiles, nullptr);
}

// one piece [lo, e) of the union of a set, lo < e <= seq_len: pieces are disjoint, so a window's edge sum never exceeds W
__device__ __forceinline__ void add_piece(const Acc& A, int set, unsigned long long base, uint32_t W, uint32_t lo, uint32_t e) {
  const uint32_t k0 = lo / W, k1 = (e - 1) / W;
  if (k0 == k1) {
    atomicAdd(&A.edge_cov[set][base + k0], e - lo);
    return;
  }
  atomicAdd(&A.edge_cov[set][base + k0], (uint32_t)((k0 + 1ull) * W - lo));
  atomicAdd(&A.edge_cov[set][base + k1], (uint32_t)(e - (unsigned long long)k1 * W));
  if (k1 > k0 + 1) {
    atomicAdd(&A.dcov[set][base + k0 + 1], 1ull);
    atomicAdd(&A.dcov[set][base + k1], ~0ull);
  }
}

// Every lane of the wavefront calls this: v = {records, bases, matches} to add at table slot `slot` (EMPTY: nothing).  Runs of one
// slot along the lanes are summed towards the run's first lane, which adds them to count / depth / matches
__device__ __forceinline__ void fold_add(unsigned long long slot, unsigned long long (&v)[3], unsigned long long* __restrict__ count,
                                         unsigned long long* __restrict__ depth, unsigned long long* __restrict__ matches) {
  if (__ballot(slot != EMPTY) == 0) return;  // (wavefront-uniform)
  const int lane = threadIdx.x & 63;
  const unsigned long long before = __shfl_up(slot, 1);
  const bool first_lane = lane == 0 || slot != before;
  const int end = run_end(__ballot(first_lane), lane);
  run_sum(v, lane, end);
  if (first_lane && slot != EMPTY) {
    atomicAdd(&count[slot], v[0]);
    if (v[1]) atomicAdd(&depth[slot], v[1]);
    if (v[2]) atomicAdd(&matches[slot], v[2]);
  }
}

// [a, b) lies inside its sequence (the keys kernel looked, and the host refused the call otherwise): base + k1 < T
__global__ __launch_bounds__(TB) void windows_walk_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry, uint64_t ntiles,
                                                          uint32_t scanned, uint32_t sentinel, const uint32_t* __restrict__ weight,
                                                          const unsigned long long* __restrict__ incl, uint32_t W, Acc A) {
  __shared__ unsigned long long l_wave[2][WAVES];
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint64_t k[ITEMS];
  uint32_t v[ITEMS], e[ITEMS];
  load_tile(keys, vals, n, p0, k, v);
  load_ends(ends, n, p0, e);
  bool counted[ITEMS];
  unsigned long long t_max[2] = {0, 0};  // ALL, KEPT
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    counted[j] = p0 + j < n && (uint32_t)(k[j] >> 32) != sentinel;
    if (counted[j]) {
      const unsigned long long P = (k[j] & 0xffffffff00000000ull) | e[j];
      t_max[0] = max64(t_max[0], P);
      if (v[j] & KEPT_FLAG) t_max[1] = max64(t_max[1], P);
    }
  }
  unsigned long long r[2];
  running_max_before<2>(t_max, l_wave, carry, ntiles, scanned, r);
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {  // (every lane goes through every round: fold_add talks along the wavefront)
    unsigned long long slot0 = EMPTY, slot1 = EMPTY, first[3] = {0, 0, 0}, last[3] = {0, 0, 0};
    bool kept = false;
    if (counted[j]) {
      const uint32_t seq = (uint32_t)(k[j] >> 32), a = (uint32_t)k[j], b = e[j];  // a < b <= seq_len
      const unsigned long long P = (k[j] & 0xffffffff00000000ull) | b;
      const unsigned long long base = base_of(incl, seq);
      const uint32_t k0 = a / W, k1 = (b - 1) / W, len = b - a, m = weight[v[j] & INDEX_MASK];  // (values are the indices the keys kernel wrote: < n)
      kept = (v[j] & KEPT_FLAG) != 0;
      slot0 = base + k0, slot1 = base + k1;
      first[0] = last[0] = 1;
      unsigned long long c = 0;
      if (k0 == k1) {
        first[1] = len, first[2] = m;
      } else {
        const unsigned long long ov0 = (k0 + 1ull) * W - a, ov1 = b - (unsigned long long)k1 * W;  // 1 .. W each
        first[1] = ov0, first[2] = ov0 * m / len;  // (both factors below 2^32)
        last[1] = ov1, last[2] = ov1 * m / len;
        if (k1 > k0 + 1) c = (unsigned long long)W * m / len;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 1 && !kept) continue;
        if (k1 > k0 + 1) {  // the windows between the two lie inside the record
          atomicAdd(&A.dfull[s][slot0 + 1], 1ull);
          atomicAdd(&A.dfull[s][slot1], ~0ull);
          atomicAdd(&A.dm[s][slot0 + 1], c);
          atomicAdd(&A.dm[s][slot1], 0ull - c);
        }
        const uint32_t before = (uint32_t)(r[s] >> 32) == seq ? (uint32_t)r[s] : 0u;  // the maximum of an earlier sequence is no cover here
        const uint32_t lo = a > before ? a : before;
        if (b > lo) add_piece(A, s, base, W, lo, b);
        r[s] = max64(r[s], P);
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bool in = s == 0 || kept;
      unsigned long long f[3] = {first[0], first[1], first[2]}, l[3] = {last[0], last[1], last[2]};
      fold_add(in ? slot0 : EMPTY, f, A.starts[s], A.edge_depth[s], A.edge_matches[s]);
      fold_add(in ? slot1 : EMPTY, l, A.ends[s], A.edge_depth[s], A.edge_matches[s]);
    }
  }
}

// ---- the rows and the summary ----------------------------------------------------------------------------------------------------
// the sequence of window t < T: the first one whose inclusive count lies beyond t (an unlisted sequence has the count of the one before)
__device__ __forceinline__ uint32_t seq_of(const unsigned long long* __restrict__ incl, uint32_t n_seq, unsigned long long t) {
  uint32_t lo = 0, hi = n_seq - 1;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (incl[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// starts, ends and the three difference arrays are scanned.  sets: 2 with a status, else 1 (the KEPT arrays are all zero then).
// rows: nullptr = nobody takes them.  sums: the window's empty / covered / depth / matches replace edge_depth / dcov / dfull / dm
// at t, which this lane alone reads (`ends` is read at t - 1 too, and `starts` is kept for the records of the summary)
__global__ __launch_bounds__(TB) void windows_rows_kernel(uint64_t T, uint32_t n_seq, const unsigned long long* __restrict__ incl,
                                                          const uint32_t* __restrict__ seq_len, uint32_t W, int sets, Acc A, swg_window_row* __restrict__ rows,
                                                          bool sums) {
  const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (t >= T) return;
  const uint32_t s = seq_of(incl, n_seq, t);
  const unsigned long long k = t - base_of(incl, s), start = k * W, len = seq_len[s];
  swg_window_row row;
  row.seq = s, row.index = (uint32_t)k;
  row.start = (uint32_t)start, row.end = (uint32_t)(start + W < len ? start + W : len);
#pragma unroll
  for (int set = 0; set < 2; ++set) {
    row.n[set] = (uint32_t)(A.starts[set][t] - (t ? A.ends[set][t - 1] : 0ull));
    row.depth[set] = A.edge_depth[set][t] + (unsigned long long)W * A.dfull[set][t];
    row.matches[set] = A.edge_matches[set][t] + A.dm[set][t];
    row.covered[set] = (uint32_t)(A.edge_cov[set][t] + (unsigned long long)W * A.dcov[set][t]);
    if (sums) {
      A.edge_depth[set][t] = set < sets && row.covered[set] == 0 ? 1ull : 0ull;
      A.dcov[set][t] = row.covered[set], A.dfull[set][t] = row.depth[set], A.dm[set][t] = row.matches[set];
    }
  }
  if (rows) rows[t] = row;
}

__device__ __forceinline__ unsigned long long range_sum(const unsigned long long* __restrict__ prefix, unsigned long long a, unsigned long long e) {
  return prefix[e - 1] - (a ? prefix[a - 1] : 0ull);
}

// list[j]: listed sequence j; A: the inclusive sums of what windows_rows left, and of the starts
__global__ __launch_bounds__(TB) void windows_seqs_kernel(uint64_t n_listed, const uint32_t* __restrict__ list, const unsigned long long* __restrict__ incl, Acc A,
                                                          swg_window_seq* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= n_listed) return;
  const uint32_t s = list[j];
  const unsigned long long a = base_of(incl, s), e = incl[s];  // (a listed sequence has a window: a < e)
  swg_window_seq o;
  o.seq = s, o.windows = (uint32_t)(e - a);
#pragma unroll
  for (int set = 0; set < 2; ++set) {
    o.empty[set] = (uint32_t)range_sum(A.edge_depth[set], a, e);
    o.covered[set] = range_sum(A.dcov[set], a, e);
    o.depth[set] = range_sum(A.dfull[set], a, e);
    o.matches[set] = range_sum(A.dm[set], a, e);
    o.records[set] = range_sum(A.starts[set], a, e);
  }
  out[j] = o;
}

inline unsigned blocks_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

inline int sum_scan(swg_ctx* ctx, unsigned long long* a, uint64_t count) {
  return swg_inclusive_sum_scan_u64(ctx, reinterpret_cast<uint64_t*>(a), reinterpret_cast<uint64_t*>(a), count);
}

// inside an arena frame.  vec_rows / vec_seqs: library-owned storage instead of the request's arrays (swg_paf_windows)
int windows_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const Cols& d, swg_windows_request* req, std::vector<swg_window_row>* vec_rows,
                   std::vector<swg_window_seq>* vec_seqs) {
  hipStream_t st = ctx->stream;
  const bool want_rows = (req->want & SWG_WINDOWS_ROWS) != 0, want_summary = (req->want & SWG_WINDOWS_SUMMARY) != 0;
  const uint32_t W = req->window, other = req->other_genome;
  const int sets = d.status ? 2 : 1;
  const uint64_t ntiles = (n + TILE - 1) / TILE;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  uint64_t* keys = swg_alloc<uint64_t>(ctx, n);
  uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n);
  uint32_t* vals = swg_alloc<uint32_t>(ctx, n);
  uint32_t* vals_alt = swg_alloc<uint32_t>(ctx, n);
  uint32_t* ends = swg_alloc<uint32_t>(ctx, n);
  unsigned long long* tile_max = swg_alloc<unsigned long long>(ctx, 2 * ntiles);
  unsigned long long* incl = swg_alloc<unsigned long long>(ctx, n_seq);
  uint8_t* listed = swg_alloc<uint8_t>(ctx, n_seq);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  SWG_HIP(ctx, hipMemsetAsync(scalars + D_BAD_END, 0xff, sizeof(unsigned long long), st));
  SWG_HIP(ctx, hipMemsetAsync(listed, 0, n_seq, st));
  SWG_LAUNCH(ctx, "windows_keys", windows_keys_kernel<<<grid_for(ctx, n), TB, 0, st>>>(n, d, n_seq, G, other, keys, vals, listed, scalars));
  SWG_KERNEL_CHECK(ctx);
  uint64_t h[2];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 2));
  if (h[D_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: a sequence id >= n_seq or a genome id >= n_genome");
  if (h[D_BAD_END] != ~0ull)
    return swg_set_error(ctx, SWG_ERR_INVALID, "windows: record %llu takes part and ends beyond its sequence (seq_len)", (unsigned long long)h[D_BAD_END]);

  // the window table's shape
  SWG_LAUNCH(ctx, "windows_counts", windows_counts_kernel<<<blocks_of(n_seq), TB, 0, st>>>(n_seq, listed, d.seq_len, W, incl));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(sum_scan(ctx, incl, n_seq));
  uint64_t T = 0, n_listed = 0;
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(incl + (n_seq - 1)), &T, 1));
  if (T >= MAX_WINDOWS) return swg_set_error(ctx, SWG_ERR_RANGE, "windows: 2^31 windows or more in the listed sequences (%llu)", (unsigned long long)T);
  if (T == 0) return SWG_OK;  // no record takes part: nothing is listed (the outputs are zeroed)
  swg_flag_scan fs{};
  SWG_TRY(swg_flags_count(ctx, listed, n_seq, &fs, reinterpret_cast<uint64_t*>(scalars + D_COUNT)));
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_COUNT), &n_listed, 1));
  if (want_rows) req->n_rows = T;
  if (want_summary) req->n_seqs = n_listed;
  const bool take_rows = want_rows && (vec_rows || (req->rows && T <= req->capacity));
  const bool take_seqs = want_summary && (vec_seqs || (req->seqs && n_listed <= req->seq_capacity));
  if (!take_rows && !take_seqs) return SWG_OK;  // (nobody takes anything: the counts alone)

  // the table: 14 arrays of 8-byte words and 2 of 4-byte ones, in one block each, all zero
  const size_t words = 14 * (size_t)T;
  unsigned long long* block = swg_alloc<unsigned long long>(ctx, words);
  uint32_t* cov_block = swg_alloc<uint32_t>(ctx, 2 * (size_t)T);
  swg_window_row* rows = take_rows ? swg_alloc<swg_window_row>(ctx, T) : nullptr;
  SWG_CHECK_ARENA(ctx);
  Acc A{};
  {
    unsigned long long* at = block;
    for (int s = 0; s < 2; ++s) {
      for (unsigned long long** arr : {&A.starts[s], &A.ends[s], &A.dfull[s], &A.dm[s], &A.dcov[s], &A.edge_depth[s], &A.edge_matches[s]}) *arr = at, at += T;
      A.edge_cov[s] = cov_block + (size_t)s * T;
    }
  }
  SWG_HIP(ctx, hipMemsetAsync(block, 0, words * sizeof(unsigned long long), st));
  SWG_HIP(ctx, hipMemsetAsync(cov_block, 0, 2 * (size_t)T * sizeof(uint32_t), st));

  // the sorted order and the walk over it
  {
    swg_prof_scope scope(ctx, "windows_sort");
    SWG_TRY(swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, n, 0, 32 + swg_bits_for(n_seq)));
  }
  SWG_LAUNCH(ctx, "windows_gather", windows_gather_kernel<<<(unsigned)ntiles, TB, 0, st>>>(n, keys, vals, d.b, n_seq, ends, tile_max, ntiles));
  SWG_KERNEL_CHECK(ctx);
  for (int s = 0; s < sets; ++s)
    SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max + s * ntiles), reinterpret_cast<uint64_t*>(tile_max + s * ntiles), ntiles));
  SWG_LAUNCH(ctx, "windows_walk", windows_walk_kernel<<<(unsigned)ntiles, TB, 0, st>>>(n, keys, vals, ends, tile_max, ntiles, sets == 2 ? 3u : 1u, n_seq, d.m, incl, W, A));
  SWG_KERNEL_CHECK(ctx);

  // the prefixes, the rows
  for (int s = 0; s < sets; ++s)
    for (unsigned long long* arr : {A.starts[s], A.ends[s], A.dfull[s], A.dm[s], A.dcov[s]}) SWG_TRY(sum_scan(ctx, arr, T));
  SWG_LAUNCH(ctx, "windows_rows", windows_rows_kernel<<<blocks_of(T), TB, 0, st>>>(T, n_seq, incl, d.seq_len, W, sets, A, rows, take_seqs));
  SWG_KERNEL_CHECK(ctx);
  if (take_rows) {
    swg_window_row* dst;
    SWG_TRY(rows_hand_over(ctx, rows, T, vec_rows, req->rows, req->capacity, &dst));
  }
  if (take_seqs) {
    for (int s = 0; s < sets; ++s)  // (without a status the KEPT arrays are zero, and so are their sums)
      for (unsigned long long* arr : {A.edge_depth[s], A.dfull[s], A.dm[s], A.dcov[s]}) SWG_TRY(sum_scan(ctx, arr, T));
    uint32_t* list = swg_alloc<uint32_t>(ctx, n_listed);
    swg_window_seq* seqs = swg_alloc<swg_window_seq>(ctx, n_listed);
    SWG_CHECK_ARENA(ctx);
    SWG_TRY(swg_flags_compact(ctx, fs, list));
    SWG_LAUNCH(ctx, "windows_seqs", windows_seqs_kernel<<<blocks_of(n_listed), TB, 0, st>>>(n_listed, list, incl, A, seqs));
    SWG_KERNEL_CHECK(ctx);
    swg_window_seq* dst;
    SWG_TRY(rows_hand_over(ctx, seqs, n_listed, vec_seqs, req->seqs, req->seq_capacity, &dst));
  }
  return SWG_OK;
}

// the seams' argument checks, then the device work inside an arena frame
int windows_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                const uint8_t* status, swg_windows_request* req, std::vector<swg_window_row>* vec_rows, std::vector<swg_window_seq>* vec_seqs) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: NULL records or request");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: reserved must be 0");
  if (req->want == 0 || req->want >> 2) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: want names nothing, or a bit beyond the two");
  if (req->axis > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: axis is 0 (query) or 1 (target)");
  if (req->window == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: the window size is at least 1");
  if (req->other_genome != SWG_WINDOWS_ANY && req->other_genome >= n_genome)
    return swg_set_error(ctx, SWG_ERR_INVALID, "windows: other_genome is a genome id < n_genome or SWG_WINDOWS_ANY");
  const uint64_t n = rec->n;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "windows: 2^31 records or more in one call");
  if (rec->n_seq > (uint32_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "windows: more than 2^31 sequences");
  const bool t = req->axis != 0;
  const uint32_t* weight = req->weight ? req->weight : rec->matches;
  if (n) {
    if (!rec->q_id || !rec->t_id || !(t ? rec->t_start : rec->q_start) || !(t ? rec->t_end : rec->q_end) || !seq_len || !seq_genome)
      return swg_set_error(ctx, SWG_ERR_INVALID, "windows: NULL column (q_id, t_id, the axis' two coordinates, seq_len and seq_genome are read)");
    if (!weight) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: neither a weight nor a matches column");
    if (rec->n_seq == 0 || n_genome == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "windows: records without sequences or genomes");
  }
  // (every refusal of the arguments lies above: none of them touches the caller's outputs)
  if (req->want & SWG_WINDOWS_ROWS) {
    req->n_rows = 0;
    if (vec_rows) vec_rows->clear();
  }
  if (req->want & SWG_WINDOWS_SUMMARY) {
    req->n_seqs = 0;
    if (vec_seqs) vec_seqs->clear();
  }
  if (n == 0) return SWG_OK;
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 64 + (size_t)rec->n_seq * 32 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    Cols d{t ? rec->t_id : rec->q_id, t ? rec->q_id : rec->t_id, t ? rec->t_start : rec->q_start, t ? rec->t_end : rec->q_end, weight, seq_genome, seq_len, status};
    if (!on_device) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&d.s_id, &d.o_id, &d.a, &d.b, &d.m}) s.add(col, n);
      s.add(&d.seq_genome, rec->n_seq);
      s.add(&d.seq_len, rec->n_seq);
      s.add(&d.status, n);
      SWG_TRY(s.run());
    }
    return windows_device(ctx, n, rec->n_seq, n_genome, d, req, vec_rows, vec_seqs);
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                const uint8_t* status, swg_windows_request* req) {
  try {
    return windows_run(ctx, rec, on_device, seq_len, seq_genome, n_genome, status, req, nullptr, nullptr);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

extern "C" int swg_windows_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                                   const uint8_t* status, swg_windows_request* req) {
  return records_abi(ctx, rec, false, seq_len, seq_genome, n_genome, status, req);
}

extern "C" int swg_windows_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                                          const uint8_t* status, swg_windows_request* req) {
  return records_abi(ctx, rec, true, seq_len, seq_genome, n_genome, status, req);
}

// The window texts of an open PAF: records, matches (column 10) and genome map from the handle (the last-'#' map of
// swg_paf_breadth), lengths by the last-seen rule of swg_paf_components, rows and summary from ONE device call, the formatting in
// host/windows_text.cpp.  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_windows(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t axis, uint32_t window, const char* other_genome,
                               char* out_text[2], uint64_t out_len[2]) {
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_windows: NULL argument");
  const bool wanted[2] = {out_text[0] != nullptr, out_text[1] != nullptr};
  out_text[0] = out_text[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_windows: neither text is asked for");
  if (axis > 1) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_windows: axis is 0 (query) or 1 (target)");
  if (window == 0) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_windows: the window size is at least 1");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))  // (before the context is looked at)
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "swg_paf_windows: the file has a value >= 2^32, its columns are rebased: the windows of 64-bit columns are not supported");
  const uint64_t n = swg_paf_records(p)->n;
  try {
    std::vector<std::string> gname;
    swg_paf_stats_genome_names(p, &gname);
    uint32_t other = SWG_WINDOWS_ANY;
    if (other_genome && n) {  // (a PAF without records has no genomes and gives the headers whatever the name)
      const std::string name(other_genome);
      for (size_t g = 0; g < gname.size() && other == SWG_WINDOWS_ANY; ++g)
        if (gname[g] == name || gname[g] == name + "#") other = (uint32_t)g;
      if (other == SWG_WINDOWS_ANY) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_windows: unknown genome '%s'", other_genome);
    }
    if (n && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_windows: NULL context");
    std::vector<swg_window_row> rows;
    std::vector<swg_window_seq> seqs;
    std::vector<uint32_t> seq_len, col10;  // (rec.matches may point into col10)
    if (n) {
      swg_records rec{};
      const uint32_t* seq_genome = nullptr;
      SWG_TRY(swg_paf_stats_prepare(p, &rec, &col10, &seq_genome));
      SWG_TRY(swg_paf_seq_last_lengths(p, &seq_len));
      swg_windows_request req{};
      req.axis = axis, req.window = window, req.other_genome = other;
      req.want = (wanted[0] ? SWG_WINDOWS_ROWS : 0u) | (wanted[1] ? SWG_WINDOWS_SUMMARY : 0u);
      const int rc = windows_run(ctx, &rec, false, seq_len.data(), seq_genome, rec.n_genome_last, status, &req, &rows, &seqs);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    }
    const std::string text[2] = {wanted[0] ? swg_windows_rows_text(p, rows) : std::string(),
                                 wanted[1] ? swg_windows_summary_text(p, seq_len, seqs) : std::string()};
    return texts_hand_over(text, wanted, 2, out_text, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
