// Divergence: per fixed window of W bases along every sequence that carries a record of the set, the exact
// aligned columns, matches, mismatches, M columns, unaligned and inserted bases, mismatch runs and indels of the set's CIGARs.  The
// parse, the four prefix sums, op_first[] and the entry states are cigar_build's (swg_cigar_build.h), the kind byte per op is the
// difference list's (swg_diffs_letters.h), the dense window table and its constant-updates-per-interval plan are the windows'
// (swg_windows.hip); include/sweepga_gpu.h states the definitions, swg_divergence_walk.h holds the rules.
//
// An entry of state 0 consumes exactly [a, b) of its axis sequence, so every axis base under it is in an aligned column or faces a
// gap: per window aligned = ov - unaligned and matches = aligned - mismatches - m_columns, with ov the overlap of [a, b) with the
// window.  '=' ops are never visited.
//
//   divergence_listing  one pass over the n records: the id checks, who takes part, the smallest record that ends beyond its
//                       sequence, the listed byte per sequence (every writer stores 1) and the records per sequence, counted in a
//                       register while a thread's records stay on one sequence, then folded along the wavefront before the atomic.
//   divergence_counts   K_s of every listed sequence, 0 for the others; swg_inclusive_sum_scan_u64 gives base[s] and T.  The host
//                       refuses T >= 2^31 here, before anything of that size is allocated.
//   divergence_letters  the kind byte per op.
//   divergence_entries  one thread per entry: usable or not (state 0, in the set, takes part), one 16-byte word for the op pass
//                       (table slot of window 0 of its axis sequence, origin, b, flags), and the updates for ov and n: the edges at
//                       k0 and k1, a "full" difference at k0 + 1 / k1, `starts` at k0, `ends` at k1; neighbours that hit one slot
//                       are folded along the wavefront.
//   divergence_ops      a tile of 1,024 ops per work-group, 4 consecutive ones per thread, the entry found as diffs_ops finds it.
//                       An op inside one window accumulates in six registers while the slot stays the same; the thread's last slot
//                       is folded along the wavefront by runs of one slot and the run heads issue the atomics.  An op that crosses
//                       a window border adds its edges and a "full" difference of its own quantity, one by one.
//   (scans)             swg_inclusive_sum_scan_u64 over starts, ends and the four difference arrays.
//   divergence_rows     one lane per window: its sequence by binary search, aligned and matches derived, the row written; with the
//                       summary it leaves the window's eight values in arrays that this lane alone has read,
//   (scans)             which are summed, and
//   divergence_seqs     one lane per listed sequence takes the differences of those sums, and of the starts' prefix (the entries),
//                       at its two ends.
//
// No work-group waits for another inside a launch; integer atomics only (64-bit adds, one 64-bit minimum, one or), all commutative:
// the result depends on neither record order nor launch shape.  The 64-bit differences wrap modulo 2^64; every true prefix is below
// 2^63.
//
// Device memory, from the arena: the build's; 1 byte per op (kind); 16 per entry (its word); 17 per sequence (listed byte, window
// prefix, records); 104 per window (13 arrays of 8-byte words) plus 80 for its row; 4 + 88 per listed sequence with the summary.
// The host seam stages 26 bytes per record, 8 per sequence and the set.
#include <new>
#include <vector>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "swg_cigar_build.h"
#include "swg_diffs_letters.h"
#include "swg_divergence_walk.h"
#include "host/host_internal.h"

namespace {

using namespace swg_cigar;
using namespace swg_divergence;
using swg_lift_ix::LiftCols;
using swg_pair_table::EMPTY;
using swg_pair_table::NONE32;
using swg_pair_table::reserve_first;
using swg_pair_table::run_end;
using swg_pair_table::run_sum;
using swg_pair_table::TB;
using swg_union_tiles::rows_hand_over;

static_assert(sizeof(swg_divergence_row) == 80 && sizeof(swg_divergence_seq) == 88 && sizeof(swg_divergence_request) == 104 &&
                  sizeof(swg_divergence_counts) == 56,
              "include/sweepga_gpu.h states these sizes");
enum { F_BAD_ID = C_BUILD_TOTAL, F_BAD_END, F_USABLE, F_LISTED, F_TOTAL };
constexpr uint64_t MAX_WINDOWS = uint64_t(1) << 31;
// the window table: ARRAYS arrays of T 8-byte words in one block, array i at block + i * T
enum {
  A_STARTS = 0, A_ENDS, A_FULL, A_EDGE_OV,  // entries whose first / last window this is, entries that fill it, what first and last windows add
  A_OPS,                                    // Q_OPS arrays in the order of swg_divergence_walk.h: the edges of the three extents, the three point sums
  A_DIFF = A_OPS + Q_OPS,                   // the "full" differences of the three extents
  ARRAYS = A_DIFF + Q_EXTENT
};

struct Table {
  unsigned long long* block;
  uint64_t T;
  __host__ __device__ unsigned long long* at(int array) const { return block + (uint64_t)array * T; }
};

unsigned blocks_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

int sum_scan(swg_ctx* ctx, unsigned long long* a, uint64_t count) {
  return swg_inclusive_sum_scan_u64(ctx, reinterpret_cast<uint64_t*>(a), reinterpret_cast<uint64_t*>(a), count);
}

// Every lane of the wavefront calls this: v = what to add at `slot` (EMPTY: nothing).  Runs of one slot along the lanes are summed
// towards the run's first lane; true on the first lane of a run that has a slot
template <int Q>
__device__ __forceinline__ bool fold_runs(unsigned long long slot, unsigned long long (&v)[Q]) {
  if (__ballot(slot != EMPTY) == 0) return false;  // (wavefront-uniform)
  const int lane = threadIdx.x & 63;
  const unsigned long long before = __shfl_up(slot, 1);
  const bool first_lane = lane == 0 || slot != before;
  run_sum(v, lane, run_end(__ballot(first_lane), lane));
  return first_lane && slot != EMPTY;
}

struct Cols {  // by role: s = the sequence the windows lie on, o = the other one; [a, b) on s
  const uint32_t *s_id, *o_id, *a, *b, *seq_genome, *seq_len;
  const uint8_t* status;
};

__device__ __forceinline__ bool in_set(const uint8_t* __restrict__ status, uint32_t set, uint64_t i) { return set == SWG_IV_ALL || status[i] != 0; }

// ---- ids, who takes part, the listed sequences and their records ---------------------------------------------------------------------
__global__ __launch_bounds__(TB) void divergence_listing_kernel(uint64_t n, uint64_t per_group, Cols c, uint32_t n_seq, uint32_t G, uint32_t set, uint32_t other,
                                                                uint8_t* __restrict__ listed, unsigned long long* __restrict__ seq_records,
                                                                unsigned long long* __restrict__ scalars) {
  // A work-group walks a contiguous share of the records, so that a thread's records lie TB apart and stay on one sequence for long
  // where the input has any order: it counts in a register, adds when the sequence changes, and what it holds at the end is folded
  // along the wavefront.  One atomic per wavefront and round serialises on the sequence's one address.
  unsigned long long slot = EMPTY, v[1] = {0};
  const uint64_t first = (uint64_t)blockIdx.x * per_group, end = first + per_group < n ? first + per_group : n;
  for (uint64_t i = first + threadIdx.x; i < end; i += TB) {
    if (!in_set(c.status, set, i)) continue;
    const uint32_t s = c.s_id[i], o = c.o_id[i], a = c.a[i], b = c.b[i];
    const uint32_t gs = s < n_seq ? c.seq_genome[s] : NONE32, go = o < n_seq ? c.seq_genome[o] : NONE32;  // (no gather before the id is known)
    const bool wrong = gs >= G || go >= G;
    const bool takes = !wrong && gs != go && a < b && (other == SWG_WINDOWS_ANY || go == other);
    if (wrong) atomicOr(&scalars[F_BAD_ID], 1ull);
    if (!takes) continue;
    if (b > c.seq_len[s]) atomicMin(&scalars[F_BAD_END], (unsigned long long)i);
    if (!listed[s]) listed[s] = 1;  // (every writer stores the same byte; the test spares the store, not the answer)
    if (slot != s) {
      if (slot != EMPTY) atomicAdd(&seq_records[slot], v[0]);
      slot = s, v[0] = 0;
    }
    ++v[0];
  }
  if (fold_runs(slot, v)) atomicAdd(&seq_records[slot], v[0]);  // (every lane arrives here)
}

__global__ __launch_bounds__(TB) void divergence_counts_kernel(uint32_t n_seq, const uint8_t* __restrict__ listed, const uint32_t* __restrict__ seq_len, uint32_t W,
                                                               unsigned long long* __restrict__ count) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (s < n_seq) count[s] = listed[s] ? ((unsigned long long)seq_len[s] + W - 1) / W : 0ull;
}

// incl: the inclusive sums of the counts.  The first window of sequence s in the table
__device__ __forceinline__ unsigned long long base_of(const unsigned long long* __restrict__ incl, uint32_t s) { return s ? incl[s - 1] : 0ull; }

__global__ __launch_bounds__(TB) void divergence_letters_kernel(CigarSet S, int aligned, uint8_t* __restrict__ kind) {
  swg_diffs::letters_of_chunk(S, aligned, (uint64_t)blockIdx.x * TB + threadIdx.x, kind);
}

// ---- the entries: the word for the op pass, ov and n ------------------------------------------------------------------------------
// c: the columns by role, lc: by name.  The ids of every record of the set are known to be good, and no record that takes part ends
// beyond its sequence (the listing looked, the host refused the call otherwise): base + k1 < T.  words / A.block == nullptr: the
// usable entries are counted and nothing else (nobody takes the table)
__global__ __launch_bounds__(TB) void divergence_entries_kernel(CigarSet S, Cols c, LiftCols lc, uint32_t G, uint32_t set, uint32_t axis, uint32_t other, uint32_t W,
                                                                const unsigned long long* __restrict__ incl, uint4* __restrict__ words, Table A,
                                                                unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  unsigned long long slot0 = EMPTY, slot1 = EMPTY, first[2] = {0, 0}, last[2] = {0, 0};
  bool usable = false;
  if (j < S.k) {
    const uint32_t rec = S.record[j];
    uint4 word = make_uint4(0u, 0u, 0u, 0u);
    if (reinterpret_cast<const uint8_t*>(S.state)[j] == 0 && in_set(c.status, set, rec)) {
      const uint32_t s = c.s_id[rec], o = c.o_id[rec], a = c.a[rec], b = c.b[rec];
      const uint32_t gs = c.seq_genome[s], go = c.seq_genome[o];
      usable = gs != go && a < b && (other == SWG_WINDOWS_ANY || go == other);
      if (usable && A.block) {
        const unsigned long long base = base_of(incl, s);
        const bool minus = lc.strand[rec] != 0;
        word.x = (uint32_t)base;  // (T < 2^31)
        word.y = entry_origin(S.P, S.op_first[j], axis, minus, lc.start[0][rec], lc.end[0][rec], lc.start[1][rec]);
        word.z = b;
        word.w = E_USABLE | (!axis && minus ? E_DESCENDS : 0u);
        uint32_t k0, k1;
        uint64_t in0, in1;
        window_span(a, b, W, &k0, &k1, &in0, &in1);
        slot0 = base + k0, slot1 = base + k1;
        first[0] = last[0] = 1, first[1] = in0, last[1] = in1;
        if (k1 > k0 + 1) {  // the windows between the two lie inside the entry: rare, one by one
          atomicAdd(&A.at(A_FULL)[slot0 + 1], 1ull);
          atomicAdd(&A.at(A_FULL)[slot1], ~0ull);
        }
      }
    }
    if (words) words[j] = word;
  }
  const uint64_t u = __ballot(usable);
  if ((threadIdx.x & 63) == 0 && u) atomicAdd(&scalars[F_USABLE], (unsigned long long)__popcll(u));
  if (!A.block) return;  // (uniform)
  if (fold_runs(slot0, first)) {
    atomicAdd(&A.at(A_STARTS)[slot0], first[0]);
    atomicAdd(&A.at(A_EDGE_OV)[slot0], first[1]);
  }
  if (fold_runs(slot1, last)) {
    atomicAdd(&A.at(A_ENDS)[slot1], last[0]);
    if (last[1]) atomicAdd(&A.at(A_EDGE_OV)[slot1], last[1]);
  }
}

// ---- the ops ----------------------------------------------------------------------------------------------------------------------
// the last entry j in [lo, hi] with op_first[j] <= r (op_first[lo] <= r): of several entries that begin at one op all but the last
// are empty
__device__ __forceinline__ uint32_t entry_at(const uint32_t* __restrict__ op_first, uint32_t lo, uint32_t hi, uint32_t r) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (op_first[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the six sums of one slot into the table (slot < T: an op of a usable entry lies inside its entry's [a, b))
__device__ __forceinline__ void add_at(const Table& A, unsigned long long slot, const unsigned long long (&v)[Q_OPS]) {
  if (slot >= A.T) return;
#pragma unroll
  for (int q = 0; q < Q_OPS; ++q)
    if (v[q]) atomicAdd(&A.at(A_OPS + q)[slot], v[q]);
}

constexpr int OPS = 4, TILE = TB * OPS;

__global__ __launch_bounds__(TB) void divergence_ops_kernel(CigarSet S, const uint8_t* __restrict__ kind, const uint4* __restrict__ words, uint32_t axis, uint32_t W,
                                                            Table A) {
  __shared__ uint32_t l_range[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;  // (the grid covers the ops: tile0 < S.ops)
  if (threadIdx.x < 2) {
    const uint64_t edge = threadIdx.x == 0 ? tile0 : (tile0 + TILE - 1 < S.ops ? tile0 + TILE - 1 : S.ops - 1);
    l_range[threadIdx.x] = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), (uint32_t)edge);
  }
  __syncthreads();
  const uint64_t r0 = tile0 + (uint64_t)threadIdx.x * OPS;
  uint32_t kd[OPS];
  if (r0 + OPS <= S.ops) {  // (arena blocks are 16-byte aligned and r0 is a multiple of 4)
    const uchar4 w = *reinterpret_cast<const uchar4*>(kind + r0);
    kd[0] = w.x, kd[1] = w.y, kd[2] = w.z, kd[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < OPS; ++j) kd[j] = r0 + j < S.ops ? kind[r0 + j] : 0u;
  }
  unsigned long long slot = EMPTY, v[Q_OPS];
#pragma unroll
  for (int q = 0; q < Q_OPS; ++q) v[q] = 0;
  if (kd[0] | kd[1] | kd[2] | kd[3]) {  // ('='-only threads do nothing)
    const uint32_t last = l_range[1];
    uint32_t e = entry_at(S.op_first, l_range[0], last, (uint32_t)r0);
    uint32_t next = e < last ? S.op_first[e + 1] : 0xffffffffu;  // (the tile's ops end inside entry `last`)
    uint4 ew = words[e];
#pragma unroll
    for (int j = 0; j < OPS; ++j) {
      const uint64_t r = r0 + j;
      if (next <= r) {
        while (e < last && S.op_first[e + 1] <= r) ++e;
        next = e < last ? S.op_first[e + 1] : 0xffffffffu;
        ew = words[e];
      }
      if (!kd[j] || !(ew.w & E_USABLE)) continue;
      const uint64_t l64 = swg_diffs::op_length(S.P, r, kd[j]);
      if (!l64) continue;
      const uint32_t l = (uint32_t)l64;  // (an op of a state-0 entry fits its record)
      const bool extent = has_extent(kd[j], axis);
      uint32_t lo, hi, k0, k1;
      uint64_t in0, in1;
      op_where(S.P, r, axis, ew.w, ew.y, ew.z, extent, l, &lo, &hi);
      window_span(lo, hi, W, &k0, &k1, &in0, &in1);
      const unsigned long long s0 = (unsigned long long)ew.x + k0;
      if (s0 != slot) {  // (another window, or another entry's sequence)
        if (slot != EMPTY) add_at(A, slot, v);
        slot = s0;
#pragma unroll
        for (int q = 0; q < Q_OPS; ++q) v[q] = 0;
      }
      const bool snp = kd[j] == K_SNP, m = kd[j] == K_M;  // (constant indices below)
      const unsigned long long here = extent ? in0 : 0ull;
      v[Q_MISMATCHES] += snp ? here : 0ull;
      v[Q_M_COLUMNS] += m ? here : 0ull;
      v[Q_UNALIGNED] += extent && !snp && !m ? here : 0ull;
      v[Q_INSERTED] += extent ? 0ull : l;
      v[Q_RUNS] += snp;
      v[Q_INDELS] += !snp && !m;
      if (k1 != k0) {  // the op crosses a border: its last window, and the filled ones between
        const int q = extent_quantity(kd[j]);
        const unsigned long long s1 = (unsigned long long)ew.x + k1;
        if (s1 < A.T) {
          atomicAdd(&A.at(A_OPS + q)[s1], (unsigned long long)in1);
          if (k1 > k0 + 1) {
            atomicAdd(&A.at(A_DIFF + q)[s0 + 1], 1ull);
            atomicAdd(&A.at(A_DIFF + q)[s1], ~0ull);
          }
        }
      }
    }
  }
  if (fold_runs(slot, v)) add_at(A, slot, v);
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

// starts, ends, the full difference and the three extent differences are scanned.  rows: nullptr = nobody takes them.  sums: the
// window's eight values go to A_FULL (matches), A_EDGE_OV (aligned) and the six arrays of the op pass, which this lane alone reads
// (`ends` is read at t - 1 too, and `starts` is kept for the entries of the summary)
__global__ __launch_bounds__(TB) void divergence_rows_kernel(uint32_t n_seq, const unsigned long long* __restrict__ incl, const uint32_t* __restrict__ seq_len,
                                                             uint32_t W, Table A, swg_divergence_row* __restrict__ rows, bool sums) {
  const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (t >= A.T) return;
  const uint32_t s = seq_of(incl, n_seq, t);
  const unsigned long long k = t - base_of(incl, s), start = k * W, len = seq_len[s];
  swg_divergence_row row;
  row.seq = s, row.start = (uint32_t)start, row.end = (uint32_t)(start + W < len ? start + W : len);
  row.n = (uint32_t)(A.at(A_STARTS)[t] - (t ? A.at(A_ENDS)[t - 1] : 0ull));
  const unsigned long long ov = A.at(A_EDGE_OV)[t] + (unsigned long long)W * A.at(A_FULL)[t];
  row.mismatches = A.at(A_OPS + Q_MISMATCHES)[t] + (unsigned long long)W * A.at(A_DIFF + Q_MISMATCHES)[t];
  row.m_columns = A.at(A_OPS + Q_M_COLUMNS)[t] + (unsigned long long)W * A.at(A_DIFF + Q_M_COLUMNS)[t];
  row.unaligned = A.at(A_OPS + Q_UNALIGNED)[t] + (unsigned long long)W * A.at(A_DIFF + Q_UNALIGNED)[t];
  row.aligned = ov - row.unaligned;
  row.matches = row.aligned - row.mismatches - row.m_columns;
  row.inserted = A.at(A_OPS + Q_INSERTED)[t];
  row.mismatch_runs = A.at(A_OPS + Q_RUNS)[t];
  row.indels = A.at(A_OPS + Q_INDELS)[t];
  if (sums) {
    A.at(A_EDGE_OV)[t] = row.aligned, A.at(A_FULL)[t] = row.matches;
    A.at(A_OPS + Q_MISMATCHES)[t] = row.mismatches, A.at(A_OPS + Q_M_COLUMNS)[t] = row.m_columns, A.at(A_OPS + Q_UNALIGNED)[t] = row.unaligned;
  }
  if (rows) rows[t] = row;
}

__device__ __forceinline__ unsigned long long range_sum(const unsigned long long* __restrict__ prefix, unsigned long long a, unsigned long long e) {
  return prefix[e - 1] - (a ? prefix[a - 1] : 0ull);
}

// list[j]: listed sequence j; A: the inclusive sums of what divergence_rows left, and of the starts
__global__ __launch_bounds__(TB) void divergence_seqs_kernel(uint64_t n_listed, const uint32_t* __restrict__ list, const unsigned long long* __restrict__ incl,
                                                             const unsigned long long* __restrict__ seq_records, Table A, swg_divergence_seq* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= n_listed) return;
  const uint32_t s = list[j];
  const unsigned long long a = base_of(incl, s), e = incl[s];  // (a listed sequence has a window: a < e)
  swg_divergence_seq o;
  o.seq = s, o.windows = (uint32_t)(e - a);
  o.records = seq_records[s];
  o.entries = range_sum(A.at(A_STARTS), a, e);
  o.aligned = range_sum(A.at(A_EDGE_OV), a, e);
  o.matches = range_sum(A.at(A_FULL), a, e);
  o.mismatches = range_sum(A.at(A_OPS + Q_MISMATCHES), a, e);
  o.m_columns = range_sum(A.at(A_OPS + Q_M_COLUMNS), a, e);
  o.unaligned = range_sum(A.at(A_OPS + Q_UNALIGNED), a, e);
  o.inserted = range_sum(A.at(A_OPS + Q_INSERTED), a, e);
  o.mismatch_runs = range_sum(A.at(A_OPS + Q_RUNS), a, e);
  o.indels = range_sum(A.at(A_OPS + Q_INDELS), a, e);
  out[j] = o;
}

int divergence_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                   const uint8_t* status, const swg_cigar_set* cigars, swg_divergence_request* req, std::vector<swg_divergence_row>* vec_rows,
                   std::vector<swg_divergence_seq>* vec_seqs) {
  static const char* const who = "divergence";
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL records or request", who);
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: reserved must be 0", who);
  if (req->want == 0 || req->want >> 2) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: want names nothing, or a bit beyond the two", who);
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (req->axis > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: axis is 0 (query) or 1 (target)", who);
  if (req->window == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the window size is at least 1", who);
  if (req->other_genome != SWG_WINDOWS_ANY && req->other_genome >= n_genome)
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: other_genome is a genome id < n_genome or SWG_WINDOWS_ANY", who);
  if (req->set == SWG_IV_KEPT && !status) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  const uint64_t n = rec->n, k = cigars ? cigars->k : 0;
  const uint32_t n_seq = rec->n_seq, G = n_genome;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^31 records or more in one call", who);
  if (n_seq > (uint32_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: more than 2^31 sequences", who);
  uint64_t B = 0;
  SWG_TRY(cigar_set_check_host(ctx, who, cigars, on_device, n, &B));
  if (B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
  if (n) {
    if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand || !seq_len || !seq_genome)
      return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL column (the six columns, strand, seq_len and seq_genome are read)", who);
    if (n_seq == 0 || G == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: records without sequences or genomes", who);
  }
  // (every refusal of the arguments lies above: none of them touches the caller's outputs)
  req->n_rows = req->n_seqs = req->ops = req->cigar_bad = req->usable = 0;
  if (vec_rows) vec_rows->clear();
  if (vec_seqs) vec_seqs->clear();
  if (n == 0) return SWG_OK;  // no device work (a set with an entry was refused: its record is >= n)
  const bool want_rows = (req->want & SWG_DIVERGENCE_ROWS) != 0, want_summary = (req->want & SWG_DIVERGENCE_SUMMARY) != 0;
  const uint32_t W = req->window, axis = req->axis, set = req->set, other = req->other_genome;
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)(on_device ? 0 : n * 26 + (size_t)n_seq * 8) + (size_t)n_seq * 32 + (size_t)B * 24 + (size_t)k * 48 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    hipStream_t st = ctx->stream;
    LiftCols lc{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const uint32_t *d_genome = seq_genome, *d_len = seq_len;  // (the frame may run twice: what the stager replaces is the frame's own)
    CigarSet S{};
    S.k = k, S.B = B;
    if (k) S.record = cigars->record, S.offset = cigars->offset, S.text = cigars->text;
    if (!on_device) {
      swg_stager s(ctx);
      for (int a = 0; a < 2; ++a) s.add(&lc.id[a], n), s.add(&lc.start[a], n), s.add(&lc.end[a], n);
      s.add(&lc.strand, n);
      s.add(&lc.status, n);
      s.add(&d_genome, (size_t)n_seq);
      s.add(&d_len, (size_t)n_seq);
      if (k) {
        s.add(&S.record, k);
        s.add(&S.offset, k + 1);
        s.add(&S.text, B);
      }
      SWG_TRY(s.run());
    }
    const Cols c{lc.id[axis], lc.id[1 - axis], lc.start[axis], lc.end[axis], d_genome, d_len, lc.status};
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, F_TOTAL);
    unsigned long long* incl = swg_alloc<unsigned long long>(ctx, n_seq);
    unsigned long long* seq_records = swg_alloc<unsigned long long>(ctx, n_seq);
    uint8_t* listed = swg_alloc<uint8_t>(ctx, n_seq);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(scalars, 0, F_TOTAL * sizeof(unsigned long long), st));
    SWG_HIP(ctx, hipMemsetAsync(scalars + F_BAD_END, 0xff, sizeof(unsigned long long), st));
    SWG_HIP(ctx, hipMemsetAsync(seq_records, 0, (size_t)n_seq * sizeof(unsigned long long), st));
    SWG_HIP(ctx, hipMemsetAsync(listed, 0, n_seq, st));
    if (k) {
      if (on_device) {
        SWG_TRY(cigar_set_check_device(ctx, who, n, &S, scalars));
        if (S.B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
      }
      SWG_TRY(cigar_build(ctx, who, lc, &S, scalars));
    }
    const uint64_t ops = S.ops;

    // who takes part, and the window table's shape
    const swg_pair_table::Share share = swg_pair_table::share_for(ctx, n);
    SWG_LAUNCH(ctx, "divergence_listing",
               divergence_listing_kernel<<<share.grid, TB, 0, st>>>(n, share.per_group, c, n_seq, G, set, other, listed, seq_records, scalars));
    SWG_KERNEL_CHECK(ctx);
    uint64_t h[F_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, F_TOTAL));
    if (h[F_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: a record of the set has a sequence id >= n_seq or a genome id >= n_genome", who);
    if (h[F_BAD_END] != ~0ull)
      return swg_set_error(ctx, SWG_ERR_INVALID, "%s: record %llu takes part and ends beyond its sequence (seq_len)", who, (unsigned long long)h[F_BAD_END]);
    SWG_LAUNCH(ctx, "divergence_counts", divergence_counts_kernel<<<blocks_of(n_seq), TB, 0, st>>>(n_seq, listed, d_len, W, incl));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(sum_scan(ctx, incl, n_seq));
    uint64_t T = 0, n_listed = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(incl + (n_seq - 1)), &T, 1));
    if (T >= MAX_WINDOWS) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^31 windows or more in the listed sequences (%llu)", who, (unsigned long long)T);
    swg_flag_scan fs{};
    if (T) {
      SWG_TRY(swg_flags_count(ctx, listed, n_seq, &fs, reinterpret_cast<uint64_t*>(scalars + F_LISTED)));
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + F_LISTED), &n_listed, 1));
    }
    const bool take_rows = T && want_rows && (vec_rows || (req->rows && T <= req->capacity));
    const bool take_seqs = T && want_summary && (vec_seqs || (req->seqs && n_listed <= req->seq_capacity));
    const bool table = take_rows || take_seqs;

    Table A{nullptr, T};
    uint4* words = nullptr;
    uint8_t* kind = nullptr;
    swg_divergence_row* rows = nullptr;
    if (table) {
      A.block = swg_alloc<unsigned long long>(ctx, (size_t)ARRAYS * T);
      if (take_rows) rows = swg_alloc<swg_divergence_row>(ctx, T);
      if (k) words = swg_alloc<uint4>(ctx, k);
      if (ops) kind = swg_alloc<uint8_t>(ctx, ops + 1);
      SWG_CHECK_ARENA(ctx);
      SWG_HIP(ctx, hipMemsetAsync(A.block, 0, (size_t)ARRAYS * T * sizeof(unsigned long long), st));
    }
    if (k && T) {  // (without a window nothing takes part: no entry is usable)
      SWG_LAUNCH(ctx, "divergence_entries", divergence_entries_kernel<<<blocks_of(k), TB, 0, st>>>(S, c, lc, G, set, axis, other, W, incl, words, A, scalars));
      SWG_KERNEL_CHECK(ctx);
    }
    if (table && ops) {
      const int aligned = (reinterpret_cast<uintptr_t>(S.text) & 15) == 0;
      SWG_LAUNCH(ctx, "divergence_letters", divergence_letters_kernel<<<blocks_of((S.B + 15) / 16), TB, 0, st>>>(S, aligned, kind));
      SWG_KERNEL_CHECK(ctx);
      SWG_LAUNCH(ctx, "divergence_ops", divergence_ops_kernel<<<(unsigned)((ops + TILE - 1) / TILE), TB, 0, st>>>(S, kind, words, axis, W, A));
      SWG_KERNEL_CHECK(ctx);
    }
    if (table) {
      for (int a : {(int)A_STARTS, (int)A_ENDS, (int)A_FULL, A_DIFF + Q_MISMATCHES, A_DIFF + Q_M_COLUMNS, A_DIFF + Q_UNALIGNED}) SWG_TRY(sum_scan(ctx, A.at(a), T));
      SWG_LAUNCH(ctx, "divergence_rows", divergence_rows_kernel<<<blocks_of(T), TB, 0, st>>>(n_seq, incl, d_len, W, A, rows, take_seqs));
      SWG_KERNEL_CHECK(ctx);
    }
    if (take_rows) {
      swg_divergence_row* dst;
      SWG_TRY(rows_hand_over(ctx, rows, T, vec_rows, req->rows, req->capacity, &dst));
    }
    if (take_seqs) {
      for (int a = A_FULL; a < A_DIFF; ++a) SWG_TRY(sum_scan(ctx, A.at(a), T));  // matches, aligned and the six of the op pass
      uint32_t* list = swg_alloc<uint32_t>(ctx, n_listed);
      swg_divergence_seq* seqs = swg_alloc<swg_divergence_seq>(ctx, n_listed);
      SWG_CHECK_ARENA(ctx);
      SWG_TRY(swg_flags_compact(ctx, fs, list));
      SWG_LAUNCH(ctx, "divergence_seqs", divergence_seqs_kernel<<<blocks_of(n_listed), TB, 0, st>>>(n_listed, list, incl, seq_records, A, seqs));
      SWG_KERNEL_CHECK(ctx);
      swg_divergence_seq* dst;
      SWG_TRY(rows_hand_over(ctx, seqs, n_listed, vec_seqs, req->seqs, req->seq_capacity, &dst));
    }
    if (req->state && k) SWG_HIP(ctx, hipMemcpyAsync(req->state, S.state, k, hipMemcpyDeviceToHost, st));
    uint64_t out[F_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), out, F_TOTAL));  // (and the copies above are done)
    if (want_rows) req->n_rows = T;
    if (want_summary) req->n_seqs = n_listed;
    req->ops = ops, req->cigar_bad = k ? out[C_BAD_ENTRIES] : 0, req->usable = out[F_USABLE];
    return SWG_OK;
  });
}

}  // namespace

int swg_divergence_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                       const uint8_t* status, const swg_cigar_set* cigars, swg_divergence_request* req, std::vector<swg_divergence_row>* vec_rows,
                       std::vector<swg_divergence_seq>* vec_seqs) {
  try {
    return divergence_run(ctx, rec, on_device, seq_len, seq_genome, n_genome, status, cigars, req, vec_rows, vec_seqs);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_divergence_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                                      const uint8_t* status, const swg_cigar_set* cigars, swg_divergence_request* req) {
  return swg_divergence_run(ctx, rec, false, seq_len, seq_genome, n_genome, status, cigars, req, nullptr, nullptr);
}
extern "C" int swg_divergence_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint32_t* seq_genome, uint32_t n_genome,
                                             const uint8_t* status, const swg_cigar_set* cigars, swg_divergence_request* req) {
  return swg_divergence_run(ctx, rec, true, seq_len, seq_genome, n_genome, status, cigars, req, nullptr, nullptr);
}
