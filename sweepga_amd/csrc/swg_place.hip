// Placement: every sequence ordered and oriented along its best partner of each other genome -- which
// sequence of the other genome it belongs to, on which strand, and where along it -- from the record columns, seq_len,
// seq_genome and (for the KEPT set) the status column.  include/sweepga_gpu.h states the definitions.  On axis 0 the placed
// sequence s is q_id and the partner p is t_id; on axis 1 the columns swap (Cols holds them by role).
//
// Everything below is a sort, a scan, a compaction or a pass with one lane per element; no group is reduced by a loop over its
// members and no kernel carries anything across work-groups, so there is no seam for a value to depend on:
//
//   place_keys     one pass: the id checks, the records that take part, key = s << (b + 1) | p << 1 | strand (b = bits(n_seq - 1))
//                  and value = record; the others get the sentinel 1 << (2b + 1), which sorts last.
//   (sort)         swg_radix_sort_pairs over 2b + 2 bits: stable, so a run of one (s, p, strand) stays in record order.  The m
//                  records that take part are the first m positions; nothing below looks beyond them.
//   place_heads    run heads (key != the key before) and the weight of every position; swg_inclusive_sum_scan_u64 over the
//                  weights: the sum of any run is the difference of two prefixes.  The heads are compacted (swg_flags_*).
//   place_runs     a run opens a candidate (s, p) when its key >> 1 differs from the run's before; compacted again.
//   place_cands    one lane per candidate: its one or two runs give fwd, rev and n_records; key = W - bases (W = all weights).
//   (two sorts)    candidates by bases descending (stable: p ascending among equals, as they come), then by (s, g) stable: every
//                  (s, g) group lies together with its winner first and the runner-up second.  The segmented argmax is the sort.
//   place_groups   group heads and the bases in that order; a sum scan gives total_bases; place_winners takes winner, runner-up
//                  and total of each group and flags the groups whose winner has bases >= min_bases: the rows, compacted.
//   place_decide   one lane per row: orientation, the deciding run (a range of sorted positions) and the span's neutral elements.
//   place_expand   one lane per deciding record (its row by binary search over the scanned run lengths): key = row << 34 |
//                  (off + 2^32), value = record, and the span: minima and maxima meet in an LDS table of the work-group (rows
//                  ascend along the positions and every row has a record, so row - first row < TB) and leave it with one 32-bit
//                  atomicMin / atomicMax per (work-group, row, quantity).
//   (sort)         by (row, off): 34 + bits(rows - 1) bits.
//   place_weights  weights in that order; a sum scan; place_median: the one position of each row whose exclusive prefix is below
//                  half and whose inclusive prefix reaches it writes the offset (W = 0: the row's first position).
//   place_rekey    the layout order (genome of s, g, p, start, s) by three stable sorts from the low end: start + 2^33 (35 bits;
//                  the rows come in s order), p, then the genome pair.
//   place_marks    heads of the (genome of s, p) runs as position + 1, swg_inclusive_max_scan_u64: rank = position - head.
//   place_rows     gathers swg_placement; place_pairs the summary from four sum scans over the ordered rows and the compacted
//                  genome-pair heads.
//
// Device memory, from the context's arena: 24 bytes per record for the first sort (two 8-byte key and two 4-byte value buffers)
// plus the radix sort's histograms, 9 bytes per record that takes part (weight prefix, head flag), 5 per run, 73 per candidate,
// 25 per (s, g) group, 24 per deciding record (the median's sort) + 8 (weight prefix), 218 per row, 52 per genome pair.  The host
// seam stages six columns and 2 bytes per record: 26 bytes more, and 8 per sequence.  Integer arithmetic only; the atomics are 32-bit minima and
// maxima, which commute: nothing depends on record order or grid shape.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "host/host_internal.h"

namespace {

using swg_pair_table::grid_for;
using swg_pair_table::NONE32;
using swg_pair_table::reserve_first;
using swg_pair_table::TB;
using swg_pair_table::wave_sum;
using swg_union_tiles::rows_hand_over;

constexpr int OFF_BITS = 34;     // off + 2^32 lies in 1 .. 3 * 2^32 - 2
constexpr int START_BITS = 35;   // start + 2^33 lies in 2 .. 2^33 + 2^33 - 2
constexpr uint64_t MAX_ROWS = uint64_t(1) << (64 - OFF_BITS);  // the median key holds the row above the anchor
enum { D_BAD_ID = 0, D_TAKING, D_COUNT, D_TOTAL };
static_assert(sizeof(swg_placement) == 104 && sizeof(swg_place_pair) == 48 && sizeof(swg_place_request) == 72, "include/sweepga_gpu.h states these sizes");

struct Cols {  // by role: s = the placed sequence, p = the partner
  const uint32_t *s_id, *p_id, *ss, *se, *ps, *pe, *seq_genome, *seq_len;
  const uint8_t *strand, *status;  // status: nullptr = every record is in the set
};

struct Cands {  // one entry per candidate, in (s, p) order
  uint32_t *s, *p, *n_records, *first_run, *n_runs;
  unsigned long long *fwd, *rev;
};

struct Groups {  // one entry per (s, g) group
  uint32_t* winner;  // candidate
  unsigned long long *total, *runner;
};

struct Rows {  // one entry per row, in (s, g) order
  uint32_t *cand, *group, *first, *span[4];  // first: the deciding run's first sorted position; span: q_lo, q_hi, t_lo, t_hi
  unsigned long long* end;                   // inclusive scan of the deciding runs' lengths: one past the row's last deciding record
  long long* offset;
  uint8_t* orient;
};

__device__ __forceinline__ uint64_t weight_of(const Cols& c, uint32_t r) { return (uint64_t)(c.se[r] - c.ss[r]); }  // (start <= end is assumed)

__device__ __forceinline__ long long anchor_of(const Cols& c, uint32_t r) {
  return c.strand[r] ? (long long)c.pe[r] + (long long)c.ss[r] : (long long)c.ps[r] - (long long)c.ss[r];
}

// ---- ids, who takes part, the keys ---------------------------------------------------------------------------------------------
// a grid of grid_for work-groups strides over the records: one add per work-group on the call's two counters
__global__ __launch_bounds__(TB) void place_keys_kernel(uint64_t n, Cols c, uint32_t n_seq, uint32_t G, int b, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals, unsigned long long* __restrict__ scalars) {
  __shared__ unsigned long long l_taking[TB / 64];
  __shared__ uint32_t l_bad;
  if (threadIdx.x == 0) l_bad = 0;
  unsigned long long taking = 0;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TB) {
    const uint32_t s = c.s_id[i], p = c.p_id[i];
    const uint32_t gs = s < n_seq ? c.seq_genome[s] : NONE32, gp = p < n_seq ? c.seq_genome[p] : NONE32;  // (no gather before the id is known)
    const bool wrong = gs >= G || gp >= G;
    const bool takes = !wrong && gs != gp && (!c.status || c.status[i] != 0);
    keys[i] = takes ? ((uint64_t)s << (b + 1)) | ((uint64_t)p << 1) | (c.strand[i] ? 1u : 0u) : uint64_t(1) << (2 * b + 1);
    vals[i] = (uint32_t)i;
    bad |= wrong;
    taking += takes;
  }
  taking = wave_sum(taking);
  const bool any_bad = __ballot(bad) != 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    l_taking[threadIdx.x >> 6] = taking;
    if (any_bad) l_bad = 1;  // (every writer stores the same word)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < TB / 64; ++w) t += l_taking[w];
    if (t) atomicAdd(&scalars[D_TAKING], t);
    if (l_bad) atomicOr(&scalars[D_BAD_ID], 1ull);
  }
}

// ---- runs of one (s, p, strand) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void place_heads_kernel(uint64_t m, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, Cols c,
                                                         uint8_t* __restrict__ head, unsigned long long* __restrict__ w) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= m) return;
  head[i] = i == 0 || keys[i] != keys[i - 1];
  w[i] = weight_of(c, vals[i]);  // (values are the indices the keys kernel wrote: < n)
}

// runs[r]: the first position of run r.  A run opens a candidate when its (s, p) differs from the run's before
__global__ __launch_bounds__(TB) void place_runs_kernel(uint64_t n_runs, const uint32_t* __restrict__ runs, const uint64_t* __restrict__ keys,
                                                        uint8_t* __restrict__ opens) {
  const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (r >= n_runs) return;
  opens[r] = r == 0 || (keys[runs[r]] >> 1) != (keys[runs[r - 1]] >> 1);
}

// the sum of the weights over the sorted positions [a, e)
__device__ __forceinline__ unsigned long long range_sum(const unsigned long long* __restrict__ prefix, uint64_t a, uint64_t e) {
  return prefix[e - 1] - (a ? prefix[a - 1] : 0ull);
}

// list[c]: the first run of candidate c.  A candidate has one run or two ('+' before '-').  key: W - bases, so that an ascending
// sort puts the largest first
__global__ __launch_bounds__(TB) void place_cands_kernel(uint64_t n_cands, const uint32_t* __restrict__ list, uint64_t n_runs,
                                                         const uint32_t* __restrict__ runs, uint64_t m, const uint64_t* __restrict__ keys,
                                                         const unsigned long long* __restrict__ prefix, int b, unsigned long long W, Cands k,
                                                         uint64_t* __restrict__ sort_keys, uint32_t* __restrict__ sort_vals) {
  const uint64_t c = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (c >= n_cands) return;
  const uint32_t r0 = list[c];
  const uint64_t r1 = c + 1 < n_cands ? list[c + 1] : n_runs;
  unsigned long long fwd = 0, rev = 0;
  const uint64_t first = runs[r0], last = r1 < n_runs ? runs[r1] : m;
  for (uint64_t r = r0; r < r1; ++r) {  // (once or twice)
    const uint64_t a = runs[r], e = r + 1 < n_runs ? runs[r + 1] : m;
    const unsigned long long sum = range_sum(prefix, a, e);
    if (keys[a] & 1u) rev += sum; else fwd += sum;
  }
  const uint64_t key = keys[first];
  k.s[c] = (uint32_t)(key >> (b + 1));
  k.p[c] = (uint32_t)(key >> 1) & (uint32_t)((uint64_t(1) << b) - 1);
  k.fwd[c] = fwd, k.rev[c] = rev;
  k.n_records[c] = (uint32_t)(last - first);
  k.first_run[c] = r0, k.n_runs[c] = (uint32_t)(r1 - r0);
  sort_keys[c] = W - (fwd + rev);
  sort_vals[c] = (uint32_t)c;
}

// keys of the second candidate sort, in the order the first one left: (s, g)
__global__ __launch_bounds__(TB) void place_group_keys_kernel(uint64_t n_cands, const uint32_t* __restrict__ order, Cands k,
                                                              const uint32_t* __restrict__ seq_genome, int gb, uint64_t* __restrict__ sort_keys) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_cands) return;
  const uint32_t c = order[i];
  sort_keys[i] = ((uint64_t)k.s[c] << gb) | seq_genome[k.p[c]];  // (p < n_seq and its genome < G: the keys kernel checked every record)
}

__global__ __launch_bounds__(TB) void place_groups_kernel(uint64_t n_cands, const uint64_t* __restrict__ group_keys, const uint32_t* __restrict__ order,
                                                          Cands k, uint8_t* __restrict__ head, unsigned long long* __restrict__ bases) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_cands) return;
  head[i] = i == 0 || group_keys[i] != group_keys[i - 1];
  const uint32_t c = order[i];
  bases[i] = k.fwd[c] + k.rev[c];
}

// list[j]: the first position of group j in the (s, g, bases descending, p) order; prefix: the inclusive sums of the bases there
__global__ __launch_bounds__(TB) void place_winners_kernel(uint64_t n_groups, const uint32_t* __restrict__ list, uint64_t n_cands,
                                                           const uint32_t* __restrict__ order, const unsigned long long* __restrict__ prefix,
                                                           unsigned long long min_bases, Groups g, uint8_t* __restrict__ is_row) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= n_groups) return;
  const uint64_t a = list[j], e = j + 1 < n_groups ? list[j + 1] : n_cands;
  const unsigned long long best = range_sum(prefix, a, a + 1);
  g.winner[j] = order[a];
  g.total[j] = range_sum(prefix, a, e);
  g.runner[j] = a + 1 < e ? range_sum(prefix, a + 1, a + 2) : 0ull;
  is_row[j] = best >= min_bases;
}

// ---- the rows: orientation and the deciding run --------------------------------------------------------------------------------
// list[r]: the group of row r.  '+' when fwd >= rev and the winner has a '+' record, else '-'
__global__ __launch_bounds__(TB) void place_decide_kernel(uint64_t n_rows, const uint32_t* __restrict__ list, Groups g, Cands k, uint64_t n_runs,
                                                          const uint32_t* __restrict__ runs, uint64_t m, const uint64_t* __restrict__ keys, Rows R) {
  const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t j = list[r], c = g.winner[j];
  const uint32_t r0 = k.first_run[c];
  uint32_t run = r0;  // one run: the strand there is
  if (k.n_runs[c] == 2 && k.fwd[c] < k.rev[c]) run = r0 + 1;
  const uint64_t a = runs[run], e = (uint64_t)run + 1 < n_runs ? runs[run + 1] : m;
  R.cand[r] = c, R.group[r] = j, R.first[r] = (uint32_t)a;
  R.end[r] = e - a;  // (scanned afterwards)
  R.orient[r] = (uint8_t)(keys[a] & 1u);
  R.span[0][r] = R.span[2][r] = NONE32;
  R.span[1][r] = R.span[3][r] = 0;
}

// the row of deciding position d: the first row whose end lies beyond d
__device__ __forceinline__ uint32_t row_of(const unsigned long long* __restrict__ end, uint64_t n_rows, uint64_t d) {
  uint64_t lo = 0, hi = n_rows - 1;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (end[mid] > d) hi = mid; else lo = mid + 1;
  }
  return (uint32_t)lo;
}

// One lane per deciding record, in the first sort's order: rows ascend along d and every row has a record, so the rows of one
// work-group are first_row .. first_row + TB - 1 at most and the LDS table is indexed by row - first_row.
__global__ __launch_bounds__(TB) void place_expand_kernel(uint64_t n_deciding, uint64_t n_rows, Rows R, const uint32_t* __restrict__ vals, Cols c,
                                                          uint64_t* __restrict__ sort_keys, uint32_t* __restrict__ sort_vals) {
  __shared__ uint32_t l_span[4][TB];
  __shared__ uint32_t l_first_row, l_last_row;
  l_span[0][threadIdx.x] = l_span[2][threadIdx.x] = NONE32;
  l_span[1][threadIdx.x] = l_span[3][threadIdx.x] = 0;
  const uint64_t d = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const bool in = d < n_deciding;
  uint32_t row = 0, v[4] = {NONE32, 0, NONE32, 0};
  if (in) {
    row = row_of(R.end, n_rows, d);
    const uint64_t before = row ? R.end[row - 1] : 0ull;
    const uint32_t rec = vals[R.first[row] + (d - before)];  // (a sorted position < m)
    v[0] = c.ss[rec], v[1] = c.se[rec], v[2] = c.ps[rec], v[3] = c.pe[rec];
    sort_keys[d] = ((uint64_t)row << OFF_BITS) | (uint64_t)(anchor_of(c, rec) + (1ll << 32));
    sort_vals[d] = rec;
  }
  if (threadIdx.x == 0) l_first_row = row;  // (d of thread 0 is inside: the grid has no empty work-group)
  if (in && (threadIdx.x == TB - 1 || d + 1 == n_deciding)) l_last_row = row;
  __syncthreads();
  const uint32_t slot = row - l_first_row;  // < TB
  const uint32_t row0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)row);
  if (__ballot(!in || row != row0) == 0) {  // the whole wavefront in one row: fold along the lanes, one LDS atomic each
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      v[0] = min(v[0], (uint32_t)__shfl_xor(v[0], s)), v[1] = max(v[1], (uint32_t)__shfl_xor(v[1], s));
      v[2] = min(v[2], (uint32_t)__shfl_xor(v[2], s)), v[3] = max(v[3], (uint32_t)__shfl_xor(v[3], s));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&l_span[0][slot], v[0]), atomicMax(&l_span[1][slot], v[1]);
      atomicMin(&l_span[2][slot], v[2]), atomicMax(&l_span[3][slot], v[3]);
    }
  } else if (in) {
    atomicMin(&l_span[0][slot], v[0]), atomicMax(&l_span[1][slot], v[1]);
    atomicMin(&l_span[2][slot], v[2]), atomicMax(&l_span[3][slot], v[3]);
  }
  __syncthreads();
  const uint64_t mine = (uint64_t)l_first_row + threadIdx.x;  // slot threadIdx.x
  if (mine <= l_last_row) {  // (a row of this work-group: every one of them has a record here)
    atomicMin(&R.span[0][mine], l_span[0][threadIdx.x]), atomicMax(&R.span[1][mine], l_span[1][threadIdx.x]);
    atomicMin(&R.span[2][mine], l_span[2][threadIdx.x]), atomicMax(&R.span[3][mine], l_span[3][threadIdx.x]);
  }
}

__global__ __launch_bounds__(TB) void place_weights_kernel(uint64_t n_deciding, const uint32_t* __restrict__ recs, Cols c, unsigned long long* __restrict__ w) {
  const uint64_t d = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (d < n_deciding) w[d] = weight_of(c, recs[d]);
}

// keys: sorted by (row, off); prefix: inclusive sums of the weights in that order.  Exactly one position per row writes
__global__ __launch_bounds__(TB) void place_median_kernel(uint64_t n_deciding, const uint64_t* __restrict__ keys, const unsigned long long* __restrict__ prefix,
                                                          Rows R) {
  const uint64_t d = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (d >= n_deciding) return;
  const uint32_t row = (uint32_t)(keys[d] >> OFF_BITS);
  const uint64_t first = row ? R.end[row - 1] : 0ull, end = R.end[row];
  const unsigned long long base = first ? prefix[first - 1] : 0ull;
  const unsigned long long W = prefix[end - 1] - base;
  const unsigned long long half = W ? (W + 1) / 2 : 1ull;  // max(1, ceil(W / 2))
  const unsigned long long incl = prefix[d] - base, excl = d == first ? 0ull : prefix[d - 1] - base;
  if (W ? (excl < half && incl >= half) : d == first) R.offset[row] = (long long)(keys[d] & ((uint64_t(1) << OFF_BITS) - 1)) - (1ll << 32);
}

// ---- the layout ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long start_of(const Rows& R, const Cands& k, const Cols& c, uint32_t r) {
  return R.orient[r] ? R.offset[r] - (long long)c.seq_len[k.s[R.cand[r]]] : R.offset[r];
}

// stage 0: start + 2^33 (order = nullptr: the identity, and the values are written); 1: p; 2: the genome pair
__global__ __launch_bounds__(TB) void place_rekey_kernel(uint64_t n_rows, int stage, Rows R, Cands k, Cols c, int gb, uint64_t* __restrict__ sort_keys,
                                                         uint32_t* __restrict__ order) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_rows) return;
  const uint32_t r = stage ? order[i] : (uint32_t)i;
  const uint32_t cand = R.cand[r], s = k.s[cand], p = k.p[cand];
  if (stage == 0) {
    sort_keys[i] = (uint64_t)(start_of(R, k, c, r) + (1ll << 33));
    order[i] = r;
  } else if (stage == 1) {
    sort_keys[i] = p;
  } else {
    sort_keys[i] = ((uint64_t)c.seq_genome[s] << gb) | c.seq_genome[p];
  }
}

// genome_keys: the sorted keys of stage 2.  mark: position + 1 at the head of a (genome of s, p) run, else 0
__global__ __launch_bounds__(TB) void place_marks_kernel(uint64_t n_rows, const uint64_t* __restrict__ genome_keys, const uint32_t* __restrict__ order, Rows R,
                                                         Cands k, unsigned long long* __restrict__ mark, uint8_t* __restrict__ pair_head) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_rows) return;
  const bool new_pair = i == 0 || genome_keys[i] != genome_keys[i - 1];
  const bool new_partner = new_pair || k.p[R.cand[order[i]]] != k.p[R.cand[order[i - 1]]];
  pair_head[i] = new_pair;
  mark[i] = new_partner ? i + 1 : 0ull;
}

// head: the inclusive maximum of the marks.  sums: [4][n_rows] or nullptr -- reversed, length, bases, total_bases of every row
__global__ __launch_bounds__(TB) void place_rows_kernel(uint64_t n_rows, const uint32_t* __restrict__ order, const unsigned long long* __restrict__ head,
                                                        Rows R, Cands k, Groups g, Cols c, swg_placement* __restrict__ out,
                                                        unsigned long long* __restrict__ sums) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_rows) return;
  const uint32_t r = order[i], cand = R.cand[r], j = R.group[r];
  const uint32_t s = k.s[cand], p = k.p[cand];
  swg_placement row;
  row.seq = s, row.partner = p;
  row.genome = c.seq_genome[s], row.partner_genome = c.seq_genome[p];
  row.offset = R.offset[r];
  row.start = start_of(R, k, c, r);
  row.fwd = k.fwd[cand], row.rev = k.rev[cand];
  row.bases = row.fwd + row.rev;
  row.total_bases = g.total[j], row.runner_bases = g.runner[j];
  row.n_records = k.n_records[cand];
  row.q_lo = R.span[0][r], row.q_hi = R.span[1][r], row.t_lo = R.span[2][r], row.t_hi = R.span[3][r];
  row.rank = (uint32_t)(i - (head[i] - 1));
  row.orient = R.orient[r];
  row.reserved[0] = row.reserved[1] = row.reserved[2] = 0;
  out[i] = row;
  if (sums) {
    sums[i] = row.orient, sums[n_rows + i] = c.seq_len[s];
    sums[2 * n_rows + i] = row.bases, sums[3 * n_rows + i] = row.total_bases;
  }
}

// list[x]: the first ordered row of genome pair x; sums: the four inclusive scans
__global__ __launch_bounds__(TB) void place_pairs_kernel(uint64_t n_pairs, const uint32_t* __restrict__ list, uint64_t n_rows,
                                                         const swg_placement* __restrict__ rows, const unsigned long long* __restrict__ sums,
                                                         swg_place_pair* __restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (x >= n_pairs) return;
  const uint64_t a = list[x], e = x + 1 < n_pairs ? list[x + 1] : n_rows;
  swg_place_pair o;
  o.genome = rows[a].genome, o.partner_genome = rows[a].partner_genome;
  o.rows = e - a;
  o.reversed = range_sum(sums, a, e);
  o.length = range_sum(sums + n_rows, a, e);
  o.bases = range_sum(sums + 2 * n_rows, a, e);
  o.total_bases = range_sum(sums + 3 * n_rows, a, e);
  out[x] = o;
}

inline unsigned blocks_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

// the set flags of `flags` [count] as an ascending list; *n_set on the host
int compact(swg_ctx* ctx, const uint8_t* flags, uint64_t count, unsigned long long* d_count, uint32_t** list, uint64_t* n_set) {
  swg_flag_scan fs{};
  SWG_TRY(swg_flags_count(ctx, flags, count, &fs, reinterpret_cast<uint64_t*>(d_count)));
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(d_count), n_set, 1));
  *list = swg_alloc<uint32_t>(ctx, *n_set);
  SWG_CHECK_ARENA(ctx);
  return swg_flags_compact(ctx, fs, *list);
}

// one stable sort at some scale, in buffers of its own: keys / vals in, sorted out
struct SortBuffers {
  uint64_t *keys, *keys_alt;
  uint32_t *vals, *vals_alt;
  void take(swg_ctx* ctx, uint64_t count) {
    keys = swg_alloc<uint64_t>(ctx, count), keys_alt = swg_alloc<uint64_t>(ctx, count);
    vals = swg_alloc<uint32_t>(ctx, count), vals_alt = swg_alloc<uint32_t>(ctx, count);
  }
  int sort(swg_ctx* ctx, const char* label, uint64_t count, int bits) {
    swg_prof_scope scope(ctx, label);
    return swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, count, 0, bits);
  }
};

// inside an arena frame.  vec_rows / vec_pairs: library-owned storage instead of the request's arrays (swg_paf_place)
int place_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const Cols& d, swg_place_request* req, std::vector<swg_placement>* vec_rows,
                 std::vector<swg_place_pair>* vec_pairs) {
  hipStream_t st = ctx->stream;
  const bool want_rows = (req->want & SWG_PLACE_ROWS) != 0, want_summary = (req->want & SWG_PLACE_SUMMARY) != 0;
  const int b = swg_bits_for((uint64_t)n_seq - 1), gb = swg_bits_for((uint64_t)G - 1);
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  SortBuffers rs;
  rs.take(ctx, n);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  SWG_LAUNCH(ctx, "place_keys", place_keys_kernel<<<grid_for(ctx, n), TB, 0, st>>>(n, d, n_seq, G, b, rs.keys, rs.vals, scalars));
  SWG_KERNEL_CHECK(ctx);
  uint64_t h[2];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 2));
  if (h[D_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "place: a sequence id >= n_seq or a genome id >= n_genome");
  const uint64_t m = h[D_TAKING];
  if (m == 0) return SWG_OK;  // no record takes part: nothing to report (the outputs are zeroed)
  SWG_TRY(rs.sort(ctx, "place_sort", n, 2 * b + 2));

  // runs and candidates
  uint8_t* head = swg_alloc<uint8_t>(ctx, m);
  unsigned long long* wsum = swg_alloc<unsigned long long>(ctx, m);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "place_heads", place_heads_kernel<<<blocks_of(m), TB, 0, st>>>(m, rs.keys, rs.vals, d, head, wsum));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_inclusive_sum_scan_u64(ctx, reinterpret_cast<uint64_t*>(wsum), reinterpret_cast<uint64_t*>(wsum), m));
  uint64_t W = 0, n_runs = 0, n_cands = 0, n_groups = 0, n_rows = 0;
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(wsum + (m - 1)), &W, 1));
  uint32_t *runs, *cand_list, *group_list, *row_list;
  SWG_TRY(compact(ctx, head, m, scalars + D_COUNT, &runs, &n_runs));
  uint8_t* opens = swg_alloc<uint8_t>(ctx, n_runs);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "place_runs", place_runs_kernel<<<blocks_of(n_runs), TB, 0, st>>>(n_runs, runs, rs.keys, opens));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(compact(ctx, opens, n_runs, scalars + D_COUNT, &cand_list, &n_cands));
  Cands k{swg_alloc<uint32_t>(ctx, n_cands), swg_alloc<uint32_t>(ctx, n_cands), swg_alloc<uint32_t>(ctx, n_cands), swg_alloc<uint32_t>(ctx, n_cands),
          swg_alloc<uint32_t>(ctx, n_cands), swg_alloc<unsigned long long>(ctx, n_cands), swg_alloc<unsigned long long>(ctx, n_cands)};
  SortBuffers cs;
  cs.take(ctx, n_cands);
  uint8_t* group_head = swg_alloc<uint8_t>(ctx, n_cands);
  unsigned long long* bases = swg_alloc<unsigned long long>(ctx, n_cands);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "place_cands", place_cands_kernel<<<blocks_of(n_cands), TB, 0, st>>>(n_cands, cand_list, n_runs, runs, m, rs.keys, wsum, b, W, k, cs.keys, cs.vals));
  SWG_KERNEL_CHECK(ctx);

  // the winner of every (s, g): two stable sorts
  SWG_TRY(cs.sort(ctx, "place_cand_sort", n_cands, swg_bits_for(W)));
  SWG_LAUNCH(ctx, "place_group_keys", place_group_keys_kernel<<<blocks_of(n_cands), TB, 0, st>>>(n_cands, cs.vals, k, d.seq_genome, gb, cs.keys));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(cs.sort(ctx, "place_cand_sort", n_cands, b + gb));
  SWG_LAUNCH(ctx, "place_groups", place_groups_kernel<<<blocks_of(n_cands), TB, 0, st>>>(n_cands, cs.keys, cs.vals, k, group_head, bases));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_inclusive_sum_scan_u64(ctx, reinterpret_cast<uint64_t*>(bases), reinterpret_cast<uint64_t*>(bases), n_cands));
  SWG_TRY(compact(ctx, group_head, n_cands, scalars + D_COUNT, &group_list, &n_groups));
  Groups g{swg_alloc<uint32_t>(ctx, n_groups), swg_alloc<unsigned long long>(ctx, n_groups), swg_alloc<unsigned long long>(ctx, n_groups)};
  uint8_t* is_row = swg_alloc<uint8_t>(ctx, n_groups);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "place_winners", place_winners_kernel<<<blocks_of(n_groups), TB, 0, st>>>(n_groups, group_list, n_cands, cs.vals, bases, req->min_bases, g, is_row));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(compact(ctx, is_row, n_groups, scalars + D_COUNT, &row_list, &n_rows));
  if (n_rows >= MAX_ROWS) return swg_set_error(ctx, SWG_ERR_RANGE, "place: 2^30 rows or more (the median's key holds the row above a 34-bit anchor)");
  if (want_rows) req->n_rows = n_rows;
  if (n_rows == 0) return SWG_OK;
  const bool take_rows = want_rows && (vec_rows || (req->rows && n_rows <= req->capacity));
  if (!take_rows && !want_summary) return SWG_OK;  // (nobody takes the rows: they are not built)

  // the deciding records and their weighted median
  Rows R{};
  R.cand = swg_alloc<uint32_t>(ctx, n_rows), R.group = swg_alloc<uint32_t>(ctx, n_rows), R.first = swg_alloc<uint32_t>(ctx, n_rows);
  for (uint32_t*& span : R.span) span = swg_alloc<uint32_t>(ctx, n_rows);
  R.end = swg_alloc<unsigned long long>(ctx, n_rows);
  R.offset = swg_alloc<long long>(ctx, n_rows);
  R.orient = swg_alloc<uint8_t>(ctx, n_rows);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "place_decide", place_decide_kernel<<<blocks_of(n_rows), TB, 0, st>>>(n_rows, row_list, g, k, n_runs, runs, m, rs.keys, R));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_inclusive_sum_scan_u64(ctx, reinterpret_cast<uint64_t*>(R.end), reinterpret_cast<uint64_t*>(R.end), n_rows));
  uint64_t n_deciding = 0;
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(R.end + (n_rows - 1)), &n_deciding, 1));
  SortBuffers ms;
  ms.take(ctx, n_deciding);
  unsigned long long* dsum = swg_alloc<unsigned long long>(ctx, n_deciding);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "place_expand", place_expand_kernel<<<blocks_of(n_deciding), TB, 0, st>>>(n_deciding, n_rows, R, rs.vals, d, ms.keys, ms.vals));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(ms.sort(ctx, "place_median_sort", n_deciding, OFF_BITS + swg_bits_for(n_rows - 1)));
  SWG_LAUNCH(ctx, "place_weights", place_weights_kernel<<<blocks_of(n_deciding), TB, 0, st>>>(n_deciding, ms.vals, d, dsum));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_inclusive_sum_scan_u64(ctx, reinterpret_cast<uint64_t*>(dsum), reinterpret_cast<uint64_t*>(dsum), n_deciding));
  SWG_LAUNCH(ctx, "place_median", place_median_kernel<<<blocks_of(n_deciding), TB, 0, st>>>(n_deciding, ms.keys, dsum, R));
  SWG_KERNEL_CHECK(ctx);

  // the layout order, the ranks, the rows
  SortBuffers ls;
  ls.take(ctx, n_rows);
  unsigned long long* mark = swg_alloc<unsigned long long>(ctx, n_rows);
  uint8_t* pair_head = swg_alloc<uint8_t>(ctx, n_rows);
  swg_placement* rows = swg_alloc<swg_placement>(ctx, n_rows);
  unsigned long long* sums = want_summary ? swg_alloc<unsigned long long>(ctx, 4 * n_rows) : nullptr;
  SWG_CHECK_ARENA(ctx);
  const int stage_bits[3] = {START_BITS, b, 2 * gb};
  for (int stage = 0; stage < 3; ++stage) {
    SWG_LAUNCH(ctx, "place_rekey", place_rekey_kernel<<<blocks_of(n_rows), TB, 0, st>>>(n_rows, stage, R, k, d, gb, ls.keys, ls.vals));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(ls.sort(ctx, "place_layout_sort", n_rows, stage_bits[stage]));
  }
  SWG_LAUNCH(ctx, "place_marks", place_marks_kernel<<<blocks_of(n_rows), TB, 0, st>>>(n_rows, ls.keys, ls.vals, R, k, mark, pair_head));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(mark), reinterpret_cast<uint64_t*>(mark), n_rows));
  SWG_LAUNCH(ctx, "place_rows", place_rows_kernel<<<blocks_of(n_rows), TB, 0, st>>>(n_rows, ls.vals, mark, R, k, g, d, rows, sums));
  SWG_KERNEL_CHECK(ctx);
  if (take_rows) {
    swg_placement* dst;
    SWG_TRY(rows_hand_over(ctx, rows, n_rows, vec_rows, req->rows, req->capacity, &dst));
  }
  if (want_summary) {
    for (int q = 0; q < 4; ++q)
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, reinterpret_cast<uint64_t*>(sums + q * n_rows), reinterpret_cast<uint64_t*>(sums + q * n_rows), n_rows));
    uint32_t* pair_list;
    uint64_t n_pairs = 0;
    SWG_TRY(compact(ctx, pair_head, n_rows, scalars + D_COUNT, &pair_list, &n_pairs));
    swg_place_pair* pairs = swg_alloc<swg_place_pair>(ctx, n_pairs);
    SWG_CHECK_ARENA(ctx);
    SWG_LAUNCH(ctx, "place_pairs", place_pairs_kernel<<<blocks_of(n_pairs), TB, 0, st>>>(n_pairs, pair_list, n_rows, rows, sums, pairs));
    SWG_KERNEL_CHECK(ctx);
    req->n_pairs = n_pairs;
    swg_place_pair* dst;
    SWG_TRY(rows_hand_over(ctx, pairs, n_pairs, vec_pairs, req->pairs, req->pair_capacity, &dst));
  }
  return SWG_OK;
}

// the seams' argument checks, then the device work inside an arena frame
int place_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
              const uint8_t* status, swg_place_request* req, std::vector<swg_placement>* vec_rows, std::vector<swg_place_pair>* vec_pairs) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "place: NULL records or request");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "place: reserved must be 0");
  if (req->want == 0 || req->want >> 2) return swg_set_error(ctx, SWG_ERR_INVALID, "place: want names nothing, or a bit beyond the two");
  if (req->axis > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "place: axis is 0 (query) or 1 (target)");
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "place: set is SWG_IV_ALL or SWG_IV_KEPT");
  if (!status && req->set == SWG_IV_KEPT) return swg_set_error(ctx, SWG_ERR_INVALID, "place: the KEPT set needs a status column");
  const uint64_t n = rec->n;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "place: 2^31 records or more in one call");
  if (rec->n_seq > (uint32_t(1) << 31))
    return swg_set_error(ctx, SWG_ERR_RANGE, "place: more than 2^31 sequences (sequence, partner and strand share one 64-bit sort key)");
  if (n) {
    if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand || !seq_len || !seq_genome)
      return swg_set_error(ctx, SWG_ERR_INVALID, "place: NULL column (q_id, t_id, the four coordinates, strand, seq_len and seq_genome are read)");
    if (rec->n_seq == 0 || n_genome == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "place: records without sequences or genomes");
  }
  // (every refusal of the arguments lies above: none of them touches the caller's outputs)
  if (req->want & SWG_PLACE_ROWS) {
    req->n_rows = 0;
    if (vec_rows) vec_rows->clear();
  }
  if (req->want & SWG_PLACE_SUMMARY) {
    req->n_pairs = 0;
    if (vec_pairs) vec_pairs->clear();
  }
  if (n == 0) return SWG_OK;
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 96 + (size_t)rec->n_seq * 8 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    const bool t = req->axis != 0;
    Cols d{t ? rec->t_id : rec->q_id, t ? rec->q_id : rec->t_id, t ? rec->t_start : rec->q_start, t ? rec->t_end : rec->q_end,
           t ? rec->q_start : rec->t_start, t ? rec->q_end : rec->t_end, seq_genome, seq_len, rec->strand,
           req->set == SWG_IV_KEPT ? status : nullptr};
    if (!on_device) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&d.s_id, &d.p_id, &d.ss, &d.se, &d.ps, &d.pe}) s.add(col, n);
      s.add(&d.seq_genome, rec->n_seq);
      s.add(&d.seq_len, rec->n_seq);
      s.add(&d.status, n);
      s.add(&d.strand, n);
      SWG_TRY(s.run());
    }
    return place_device(ctx, n, rec->n_seq, n_genome, d, req, vec_rows, vec_pairs);
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                const uint8_t* status, swg_place_request* req) {
  try {
    return place_run(ctx, rec, on_device, seq_len, seq_genome, n_genome, status, req, nullptr, nullptr);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

extern "C" int swg_place_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                                 const uint8_t* status, swg_place_request* req) {
  return records_abi(ctx, rec, false, seq_len, seq_genome, n_genome, status, req);
}

extern "C" int swg_place_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                                        const uint8_t* status, swg_place_request* req) {
  return records_abi(ctx, rec, true, seq_len, seq_genome, n_genome, status, req);
}

// The placement texts of an open PAF: records and genome map from the handle (the last-'#' map of swg_paf_breadth), lengths by
// the last-seen rule of swg_paf_components, rows and summary from ONE device call, the formatting in host/place_text.cpp.
// Errors: swg_alnstats_last_error().
extern "C" int swg_paf_place(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t axis, uint32_t set, uint64_t min_bases, char* out_text[2],
                             uint64_t out_len[2]) {
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_place: NULL argument");
  const bool wanted[2] = {out_text[0] != nullptr, out_text[1] != nullptr};
  out_text[0] = out_text[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_place: neither text is asked for");
  if (axis > 1) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_place: axis is 0 (query) or 1 (target)");
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_place: set is SWG_IV_ALL or SWG_IV_KEPT");
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_place: the kept set needs a status column");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))  // (before the context is looked at)
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "swg_paf_place: the file has a value >= 2^32, its columns are rebased: the placement of 64-bit columns is not supported");
  const swg_records* rec = swg_paf_records(p);
  if (rec->n && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_place: NULL context");
  try {
    std::vector<swg_placement> rows;
    std::vector<swg_place_pair> pairs;
    std::vector<std::string> gname;
    std::vector<uint32_t> seq_len;
    if (rec->n) {
      SWG_TRY(swg_paf_seq_last_lengths(p, &seq_len));
      swg_place_request req{};
      req.axis = axis, req.set = set, req.min_bases = min_bases;
      req.want = (wanted[0] ? SWG_PLACE_ROWS : 0u) | (wanted[1] ? SWG_PLACE_SUMMARY : 0u);
      const int rc = place_run(ctx, rec, false, seq_len.data(), rec->seq_genome_last, rec->n_genome_last, status, &req, &rows, &pairs);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      swg_paf_stats_genome_names(p, &gname);
    }
    const std::string text[2] = {wanted[0] ? swg_place_rows_text(p, seq_len, rows) : std::string(),
                                 wanted[1] ? swg_place_summary_text(gname, pairs) : std::string()};
    return texts_hand_over(text, wanted, 2, out_text, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
