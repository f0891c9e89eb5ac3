// Gaps: what lies between the mappings of one kept chain -- the indel at every link, and every captured
// inversion -- from the record columns plus the status and chain columns as swg_filter* writes them.  A record takes part when
// status == SWG_ST_SCAFFOLD and chain != 0; include/sweepga_gpu.h states the definitions.
//
//   gaps_max      C = the largest chain number of a record that takes part, how many take part, and the id checks.
//   gaps_strand   a dense flag per chain number, [C + 1] 32-bit words: set when a '+' record of the chain takes part (the OR is
//                 a relaxed atomic store of 1: all writers store the same word).  Dense in the chain NUMBER, as the table of
//                 swg_blocks.hip: a sparse numbering {1, 7, 2^20} pays 4 bytes for every number up to the largest.
//   gaps_keys     key = chain << 32 | q_start, value = record; records that take no part get the chain C + 1.
//   (sort)        swg_radix_sort_pairs over the 32 + bits(C + 1) key bits: stable, so equal q_start stay in index order.  The m
//                 records that take part are the first m of the sorted order; nothing below looks beyond them.
//   gaps_core     the sorted order in tiles (swg_union_tiles.h: TILE records, ITEMS consecutive ones per thread): the class of
//                 every position (core or inverted: the record's strand against its chain's flag) and the tile maximum of
//                 mark = chain << 32 | (position + 1) over the core positions.
//   (scan)        swg_inclusive_max_scan_u64 over the tile maxima: the carry across work-groups, no wait inside a launch.
//   gaps_links    the tile again.  Chains ascend along the sorted order, so the running maximum of the marks in front of a
//                 position (running_max_before) is the LAST core position before it; it is the predecessor when its high half
//                 is the position's own chain.  A run of inverted records of any length carries through: they raise no mark.
//                 Then a gather of the two records, the classification, the row flag and predecessor of the position, and (with
//                 the summary) the reductions: runs of one genome pair folded along the thread and the lanes into the LDS table
//                 of swg_pair_table.h and from there into the global one; the spectrum through an LDS histogram per work-group,
//                 flushed once.  Every position also compares its (q_id, t_id) with the position before it in the same chain.
//   (compaction)  swg_flags_count / swg_flags_compact over the row flags: the rows' positions, ascending = the row order.
//   gaps_rows     one lane per row: gather and write swg_gap_row.
//   gaps_collect  the occupied genome pairs (list_slots); the host orders them by (q_genome, t_genome).
//
// Device memory, from the context's arena: 24 bytes per record (two 8-byte key buffers, two 4-byte value buffers) plus the radix
// sort's histograms, 6 bytes per record that takes part (class, row flag, predecessor), 4 bytes per chain NUMBER, 36 bytes per
// row (its position and the row), and the genome-pair table.  The host seam stages 7 columns and 2 bytes per record: 30 bytes
// more.  Integer atomics only; no floating point; the result does not depend on record order (the index tie-break aside) or
// grid shape.
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

using namespace swg_pair_table;   // TB, WAVES, LdsTable, PairTable, run_end, run_sum, wave_sum, grid_for, reserve_first
using namespace swg_union_tiles;  // the tile of the sorted order and the running maximum

constexpr int BINS = SWG_GAPS_BINS;
enum { D_MAX_CHAIN = 0, D_TAKING, D_BAD_ID, D_TWO_PAIRS, D_ROWS, D_LISTED, D_SPECTRUM, D_TOTAL = D_SPECTRUM + 2 * BINS };
enum { Q_LINKS = 0, Q_N_INS, Q_INS_BASES, Q_N_DEL, Q_DEL_BASES, Q_N_INV, Q_INV_BASES, Q_TOTAL };
enum : uint8_t { CLS_NONE = 0, CLS_CORE = 1, CLS_INVERTED = 2 };
static_assert(sizeof(swg_gap_row) == 32 && sizeof(swg_gap_pair) == 64 && sizeof(swg_gaps_request) == 72, "include/sweepga_gpu.h states these sizes");

using SumTable = PairTable<Q_TOTAL, false>;
using SumList = PairList<Q_TOTAL, false>;

struct Cols {
  const uint32_t *q_id, *t_id, *qs, *qe, *ts, *te, *chain, *seq_genome;
  const uint8_t *strand, *status;
};

__device__ __forceinline__ uint32_t taking_chain(const Cols& c, uint64_t i) { return c.status[i] == SWG_ST_SCAFFOLD ? c.chain[i] : 0u; }

// ---- the largest chain number, the ids -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void gaps_max_kernel(uint64_t n, Cols c, uint32_t n_seq, uint32_t G, unsigned long long* __restrict__ scalars) {
  uint32_t m = 0;
  unsigned long long taking = 0;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TB) {
    const uint32_t ch = taking_chain(c, i);
    m = max(m, ch);
    taking += ch != 0;
    const uint32_t q = c.q_id[i], t = c.t_id[i];
    bad |= q >= n_seq || t >= n_seq || c.seq_genome[q < n_seq ? q : 0] >= G || c.seq_genome[t < n_seq ? t : 0] >= G;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor(m, d));
  taking = wave_sum(taking);
  const bool any_bad = __ballot(bad) != 0;
  if ((threadIdx.x & 63) == 0) {
    if (m) atomicMax(&scalars[D_MAX_CHAIN], (unsigned long long)m);
    if (taking) atomicAdd(&scalars[D_TAKING], taking);
    if (any_bad) atomicOr(&scalars[D_BAD_ID], 1ull);
  }
}

// ---- the chain's strand --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void gaps_strand_kernel(uint64_t n, Cols c, uint32_t C, uint32_t* __restrict__ plus) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t ch = taking_chain(c, i);
  if (ch == 0 || ch > C || c.strand[i] != 0) return;  // (ch <= C by gaps_max; the test keeps every index inside the table)
  __hip_atomic_store(&plus[ch], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (every writer stores the same word: no read-modify-write)
}

__global__ __launch_bounds__(TB) void gaps_keys_kernel(uint64_t n, Cols c, uint32_t C, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t ch = taking_chain(c, i);
  keys[i] = ch != 0 && ch <= C ? ((uint64_t)ch << 32) | c.qs[i] : (uint64_t)(C + 1) << 32;
  vals[i] = (uint32_t)i;
}

// ---- the sorted order, first pass: classes and tile maxima of the core marks ---------------------------------------------------
__device__ __forceinline__ void load_cls(const uint8_t* __restrict__ cls, uint64_t m, uint64_t p0, uint8_t (&v)[ITEMS]) {
  if (p0 + ITEMS <= m) {  // (arena blocks are 16-byte aligned and p0 is a multiple of 4)
    const uchar4 w = *reinterpret_cast<const uchar4*>(cls + p0);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) v[j] = p0 + j < m ? cls[p0 + j] : CLS_NONE;
  }
}

__device__ __forceinline__ unsigned long long mark_of(uint64_t key, uint64_t p) { return (key & 0xffffffff00000000ull) | (uint32_t)(p + 1); }

// m: the records that take part = the sorted positions that count
__global__ __launch_bounds__(TB) void gaps_core_kernel(uint64_t m, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       const uint8_t* __restrict__ strand, const uint32_t* __restrict__ plus, uint32_t C,
                                                       uint8_t* __restrict__ cls, unsigned long long* __restrict__ tile_max) {
  __shared__ unsigned long long l_max[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint64_t k[ITEMS];
  uint32_t v[ITEMS];
  load_tile(keys, vals, m, p0, k, v);
  unsigned long long mine = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (p0 + j >= m) continue;
    const uint32_t ch = (uint32_t)(k[j] >> 32);
    uint8_t what = CLS_NONE;
    if (ch != 0 && ch <= C) {  // (always: the first m positions are the records that take part)
      const uint32_t chain_strand = plus[ch] ? 0u : 1u;
      what = strand[v[j]] == chain_strand ? CLS_CORE : CLS_INVERTED;  // (values are the indices the keys kernel wrote: < n)
    }
    cls[p0 + j] = what;
    if (what == CLS_CORE) mine = max64(mine, mark_of(k[j], p0 + j));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine = max64(mine, __shfl_xor(mine, d));
  if (lane == 0) l_max[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < WAVES; ++w) t = max64(t, l_max[w]);
    tile_max[blockIdx.x] = t;
  }
}

// ---- a link, an inversion ------------------------------------------------------------------------------------------------------
struct Event {
  long long dq, dt, size;
  uint32_t q_lo, q_hi, t_lo, t_hi;
};

// a, b: the link's records; minus: the chain's strand
__device__ __forceinline__ Event link_of(const Cols& c, uint32_t a, uint32_t b, bool minus) {
  const uint32_t qa = c.qe[a], qb = c.qs[b];
  const uint32_t ta = minus ? c.ts[a] : c.te[a], tb = minus ? c.te[b] : c.ts[b];  // the two facing target ends
  Event e;
  e.dq = (long long)qb - (long long)qa;
  e.dt = minus ? (long long)ta - (long long)tb : (long long)tb - (long long)ta;
  e.size = e.dq - e.dt;
  e.q_lo = min(qa, qb), e.q_hi = max(qa, qb);
  e.t_lo = min(ta, tb), e.t_hi = max(ta, tb);
  return e;
}

__device__ __forceinline__ unsigned long long magnitude(long long v) { return v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v; }

__device__ __forceinline__ int spectrum_bin(unsigned long long mag) {  // bit length, the last bin taking what lies beyond
  const int bits = mag ? 64 - __builtin_clzll(mag) : 0;
  return bits < BINS ? bits : BINS - 1;
}

// ---- the sorted order, second pass: predecessors, classification, reductions ---------------------------------------------------
// emit / pred: [m] or both nullptr (no rows are asked for).  pred: the link's left record; NONE32 where the position has no link
template <bool SUMMARY>
__global__ __launch_bounds__(TB) void gaps_links_kernel(uint64_t m, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                        const uint8_t* __restrict__ cls, const unsigned long long* __restrict__ carry, Cols c,
                                                        uint32_t min_size, uint32_t G, SumTable T, uint8_t* __restrict__ emit,
                                                        uint32_t* __restrict__ pred, unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<Q_TOTAL, false> l_pairs;
  __shared__ unsigned long long l_wave[1][WAVES];
  __shared__ uint32_t l_spec[2 * BINS];
  if (SUMMARY) {
    l_pairs.clear();
    if (threadIdx.x < 2 * BINS) l_spec[threadIdx.x] = 0;
  }
  const int lane = threadIdx.x & 63;
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint64_t k[ITEMS];
  uint32_t v[ITEMS];
  uint8_t what[ITEMS];
  load_tile(keys, vals, m, p0, k, v);
  load_cls(cls, m, p0, what);
  unsigned long long mine[1] = {0};
#pragma unroll
  for (int j = 0; j < ITEMS; ++j)
    if (what[j] == CLS_CORE) mine[0] = max64(mine[0], mark_of(k[j], p0 + j));
  unsigned long long front[1];
  running_max_before<1>(mine, l_wave, carry, 0, 1u, front);  // (one set; the barrier behind the LDS clears is in here)
  unsigned long long r = front[0];
  // the position before this thread's first one, for the (q_id, t_id) comparison
  uint32_t before_chain = 0, before_q = 0, before_t = 0;
  if (p0 > 0 && p0 < m) {
    before_chain = (uint32_t)(keys[p0 - 1] >> 32);
    const uint32_t rec = vals[p0 - 1];
    before_q = c.q_id[rec], before_t = c.t_id[rec];
  }
  unsigned long long run_key = EMPTY, run[Q_TOTAL];
#pragma unroll
  for (int i = 0; i < Q_TOTAL; ++i) run[i] = 0;
  uint32_t two_pairs = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (what[j] == CLS_NONE) continue;  // (beyond m, or never: see gaps_core)
    const uint64_t p = p0 + j;
    const uint32_t ch = (uint32_t)(k[j] >> 32), b = v[j];
    const uint32_t q = c.q_id[b], t = c.t_id[b];
    if (before_chain == ch && (before_q != q || before_t != t)) two_pairs = max(two_pairs, ch);
    before_chain = ch, before_q = q, before_t = t;
    unsigned long long add[Q_TOTAL];
#pragma unroll
    for (int i = 0; i < Q_TOTAL; ++i) add[i] = 0;
    bool row = false;
    uint32_t left = NONE32;
    if (what[j] == CLS_CORE) {
      if ((uint32_t)(r >> 32) == ch) left = vals[(uint32_t)r - 1];  // (a mark's low half is a position + 1 in front of this one)
      r = max64(r, mark_of(k[j], p));
      if (left != NONE32) {
        const Event e = link_of(c, left, b, c.strand[b] != 0);  // (a core record is on its chain's strand)
        const unsigned long long mag = magnitude(e.size);
        row = mag >= min_size;
        add[Q_LINKS] = 1;
        if (row && e.size != 0) {  // (constant indices: the sums stay in registers)
          const bool ins = e.size > 0;
          add[Q_N_INS] = ins, add[Q_INS_BASES] = ins ? mag : 0;
          add[Q_N_DEL] = !ins, add[Q_DEL_BASES] = ins ? 0 : mag;
          if (SUMMARY) atomicAdd(&l_spec[(ins ? 0 : BINS) + spectrum_bin(mag)], 1u);
        }
      }
    } else {
      const uint32_t len = c.qe[b] - c.qs[b];  // (start <= end is assumed)
      row = len >= min_size;
      left = b;
      if (row) add[Q_N_INV] = 1, add[Q_INV_BASES] = len;
    }
    if (emit) emit[p] = row ? 1 : 0, pred[p] = left;
    if (SUMMARY && (add[Q_LINKS] | add[Q_N_INV])) {
      const unsigned long long key = (unsigned long long)c.seq_genome[q] * G + c.seq_genome[t];
      if (key != run_key) {  // (a chain ends inside the thread: rare)
        if (run_key != EMPTY && !l_pairs.add(run_key, run)) table_add<Q_TOTAL, false>(T, run_key, run, 0);
        run_key = key;
#pragma unroll
        for (int i = 0; i < Q_TOTAL; ++i) run[i] = 0;
      }
#pragma unroll
      for (int i = 0; i < Q_TOTAL; ++i) run[i] += add[i];
    }
  }
  if (two_pairs) atomicMax(&scalars[D_TWO_PAIRS], (unsigned long long)two_pairs);  // (an input error: no need to be cheap)
  if (!SUMMARY) return;
  // runs of one genome pair along the lanes, summed towards the run's first lane
  if (__ballot(run_key != EMPTY)) {  // wavefront-uniform
    const unsigned long long before = __shfl_up(run_key, 1);
    const bool first_lane = lane == 0 || run_key != before;
    run_sum(run, lane, run_end(__ballot(first_lane), lane));
    if (first_lane && run_key != EMPTY && !l_pairs.add(run_key, run)) table_add<Q_TOTAL, false>(T, run_key, run, 0);
  }
  __syncthreads();
  l_pairs.flush(T, 0);
  if (threadIdx.x < 2 * BINS && l_spec[threadIdx.x]) atomicAdd(&scalars[D_SPECTRUM + threadIdx.x], (unsigned long long)l_spec[threadIdx.x]);
}

// ---- the rows ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void gaps_rows_kernel(uint64_t n_rows, const uint32_t* __restrict__ list, const uint64_t* __restrict__ keys,
                                                       const uint32_t* __restrict__ vals, const uint8_t* __restrict__ cls,
                                                       const uint32_t* __restrict__ pred, Cols c, swg_gap_row* __restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_rows) return;
  const uint32_t p = list[i];  // (positions of set row flags: < m)
  const uint32_t b = vals[p], a = pred[p];
  swg_gap_row row;
  row.chain = (uint32_t)(keys[p] >> 32);
  row.left = a, row.right = b;
  row.reserved = 0;
  if (cls[p] == CLS_CORE) {
    const Event e = link_of(c, a, b, c.strand[b] != 0);
    row.q_lo = e.q_lo, row.q_hi = e.q_hi, row.t_lo = e.t_lo, row.t_hi = e.t_hi;
    row.kind = (uint8_t)(e.size > 0 ? SWG_GAP_INS : e.size < 0 ? SWG_GAP_DEL : SWG_GAP_EVEN);
    row.flags = (uint8_t)((e.dq < 0 ? 1 : 0) | (e.dt < 0 ? 2 : 0));
  } else {
    row.q_lo = c.qs[b], row.q_hi = c.qe[b], row.t_lo = c.ts[b], row.t_hi = c.te[b];
    row.kind = (uint8_t)SWG_GAP_INV;
    row.flags = 0;
  }
  rows[i] = row;
}

__global__ __launch_bounds__(TB) void gaps_collect_kernel(SumTable T, SumList L) { list_slots(T, L); }

bool gaps_hash_forced() {  // test knob: the hashed genome-pair table at any size
  const char* knob = std::getenv("SWG_GAPS_HASH");
  return knob && knob[0] == '1';
}

// inside an arena frame.  vec_rows / vec_pairs: library-owned storage instead of the request's arrays (swg_paf_gaps)
int gaps_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const Cols& d, swg_gaps_request* req, std::vector<swg_gap_row>* vec_rows,
                std::vector<swg_gap_pair>* vec_pairs) {
  hipStream_t st = ctx->stream;
  const bool want_rows = (req->want & SWG_GAPS_ROWS) != 0, want_summary = (req->want & SWG_GAPS_SUMMARY) != 0;
  const unsigned grid_n = (unsigned)((n + TB - 1) / TB);
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  SWG_LAUNCH(ctx, "gaps_max", gaps_max_kernel<<<grid_for(ctx, n), TB, 0, st>>>(n, d, n_seq, G, scalars));
  SWG_KERNEL_CHECK(ctx);
  uint64_t h[D_SPECTRUM];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 3));
  if (h[D_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "gaps: a sequence id >= n_seq or a genome id >= n_genome");
  if (h[D_MAX_CHAIN] == 0) return SWG_OK;  // no record takes part: nothing to report (the outputs are zeroed)
  if (h[D_MAX_CHAIN] >= 0xffffffffull) return swg_set_error(ctx, SWG_ERR_RANGE, "gaps: chain number 2^32 - 1 (one past the last chain has to fit 32 bits)");
  const uint32_t C = (uint32_t)h[D_MAX_CHAIN];
  const uint64_t m = h[D_TAKING], mtiles = (m + TILE - 1) / TILE;
  uint32_t* plus = swg_alloc<uint32_t>(ctx, (size_t)C + 1);
  uint64_t* keys = swg_alloc<uint64_t>(ctx, n);
  uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n);
  uint32_t* vals = swg_alloc<uint32_t>(ctx, n);
  uint32_t* vals_alt = swg_alloc<uint32_t>(ctx, n);
  uint8_t* cls = swg_alloc<uint8_t>(ctx, m);
  uint8_t* emit = want_rows ? swg_alloc<uint8_t>(ctx, m) : nullptr;
  uint32_t* pred = want_rows ? swg_alloc<uint32_t>(ctx, m) : nullptr;
  unsigned long long* tile_max = swg_alloc<unsigned long long>(ctx, mtiles);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(plus, 0, ((size_t)C + 1) * sizeof(uint32_t), st));
  SWG_LAUNCH(ctx, "gaps_strand", gaps_strand_kernel<<<grid_n, TB, 0, st>>>(n, d, C, plus));
  SWG_KERNEL_CHECK(ctx);
  SWG_LAUNCH(ctx, "gaps_keys", gaps_keys_kernel<<<grid_n, TB, 0, st>>>(n, d, C, keys, vals));
  SWG_KERNEL_CHECK(ctx);
  {
    swg_prof_scope sort_scope(ctx, "gaps_sort");
    SWG_TRY(swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, n, 0, 32 + swg_bits_for((uint64_t)C + 1)));
  }
  SWG_LAUNCH(ctx, "gaps_core", gaps_core_kernel<<<(unsigned)mtiles, TB, 0, st>>>(m, keys, vals, d.strand, plus, C, cls, tile_max));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max), reinterpret_cast<uint64_t*>(tile_max), mtiles));
  SumTable T{};
  SumList L{};
  if (want_summary) {
    const uint64_t g2 = (uint64_t)G * G;  // genome pairs that occur <= records that take part
    SWG_TRY(table_create(ctx, G, g2 < m ? g2 : m, gaps_hash_forced(), false, scalars + D_LISTED, &T, &L));
    SWG_LAUNCH(ctx, "gaps_links", gaps_links_kernel<true><<<(unsigned)mtiles, TB, 0, st>>>(m, keys, vals, cls, tile_max, d, req->min_size, G, T, emit, pred, scalars));
  } else {
    SWG_LAUNCH(ctx, "gaps_links", gaps_links_kernel<false><<<(unsigned)mtiles, TB, 0, st>>>(m, keys, vals, cls, tile_max, d, req->min_size, G, T, emit, pred, scalars));
  }
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_SPECTRUM));
  if (h[D_TWO_PAIRS])
    return swg_set_error(ctx, SWG_ERR_INVALID, "gaps: the records of chain %llu name more than one (q_id, t_id) pair", (unsigned long long)h[D_TWO_PAIRS]);
  if (want_rows) {
    uint64_t n_rows = 0;
    swg_flag_scan fs{};
    SWG_TRY(swg_flags_count(ctx, emit, m, &fs, reinterpret_cast<uint64_t*>(scalars + D_ROWS)));
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_ROWS), &n_rows, 1));
    req->n_rows = n_rows;
    if (n_rows && (vec_rows || (req->rows && n_rows <= req->capacity))) {  // (else nobody takes the rows: they are not built)
      uint32_t* list = swg_alloc<uint32_t>(ctx, n_rows);
      swg_gap_row* rows = swg_alloc<swg_gap_row>(ctx, n_rows);
      SWG_CHECK_ARENA(ctx);
      SWG_TRY(swg_flags_compact(ctx, fs, list));
      SWG_LAUNCH(ctx, "gaps_rows", gaps_rows_kernel<<<(unsigned)((n_rows + TB - 1) / TB), TB, 0, st>>>(n_rows, list, keys, vals, cls, pred, d, rows));
      SWG_KERNEL_CHECK(ctx);
      swg_gap_row* dst;
      SWG_TRY(rows_hand_over(ctx, rows, n_rows, vec_rows, req->rows, req->capacity, &dst));
    }
  }
  if (want_summary) {
    SWG_LAUNCH(ctx, "gaps_collect", gaps_collect_kernel<<<(unsigned)((T.slots + TB - 1) / TB), TB, 0, st>>>(T, L));
    SWG_KERNEL_CHECK(ctx);
    uint64_t listed = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_LISTED), &listed, 1));
    std::vector<SumList::Entry> list[1];
    SWG_TRY(list_fetch(ctx, "gaps", L, &listed, list));
    std::sort(list[0].begin(), list[0].end(), [](const SumList::Entry& a, const SumList::Entry& b) { return a.key < b.key; });
    req->n_pairs = list[0].size();
    swg_gap_pair* dst = nullptr;
    if (vec_pairs) {
      vec_pairs->resize(list[0].size());
      dst = vec_pairs->data();
    } else if (req->pairs && req->n_pairs <= req->pair_capacity) {
      dst = req->pairs;
    }
    for (size_t x = 0; dst && x < list[0].size(); ++x) {
      const SumList::Entry& e = list[0][x];
      dst[x] = swg_gap_pair{(uint32_t)(e.key / G), (uint32_t)(e.key % G), e.v[Q_LINKS], e.v[Q_N_INS], e.v[Q_INS_BASES], e.v[Q_N_DEL],
                            e.v[Q_DEL_BASES], e.v[Q_N_INV], e.v[Q_INV_BASES]};
    }
    if (req->spectrum) {
      SWG_HIP(ctx, hipMemcpyAsync(req->spectrum, scalars + D_SPECTRUM, 2 * BINS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));
    }
  }
  return SWG_OK;
}

// the seams' argument checks, then the device work inside an arena frame
int gaps_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const uint32_t* chain, const uint32_t* seq_genome,
             uint32_t n_genome, swg_gaps_request* req, std::vector<swg_gap_row>* vec_rows, std::vector<swg_gap_pair>* vec_pairs) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "gaps: NULL records or request");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "gaps: reserved must be 0");
  if (req->want == 0 || req->want >> 2) return swg_set_error(ctx, SWG_ERR_INVALID, "gaps: want names nothing, or a bit beyond the two");
  const uint64_t n = rec->n;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "gaps: 2^31 records or more in one call");
  if (n) {
    if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand || !status || !chain || !seq_genome)
      return swg_set_error(ctx, SWG_ERR_INVALID, "gaps: NULL column (q_id, t_id, the four coordinates, strand, status, chain and seq_genome are read)");
    if (rec->n_seq == 0 || n_genome == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "gaps: records without sequences or genomes");
  }
  // (every refusal of the arguments lies above: none of them touches the caller's outputs)
  if (req->want & SWG_GAPS_ROWS) {
    req->n_rows = 0;
    if (vec_rows) vec_rows->clear();
  }
  if (req->want & SWG_GAPS_SUMMARY) {
    req->n_pairs = 0;
    if (vec_pairs) vec_pairs->clear();
    if (req->spectrum) std::memset(req->spectrum, 0, 2 * BINS * sizeof(uint64_t));
  }
  if (n == 0) return SWG_OK;
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 64 + (size_t)rec->n_seq * 4 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    Cols d{rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end, chain, seq_genome, rec->strand, status};
    if (!on_device) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&d.q_id, &d.t_id, &d.qs, &d.qe, &d.ts, &d.te, &d.chain}) s.add(col, n);
      s.add(&d.seq_genome, rec->n_seq);
      s.add(&d.status, n);
      s.add(&d.strand, n);
      SWG_TRY(s.run());
    }
    return gaps_device(ctx, n, rec->n_seq, n_genome, d, req, vec_rows, vec_pairs);
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const uint32_t* chain, const uint32_t* seq_genome,
                uint32_t n_genome, swg_gaps_request* req) {
  try {
    return gaps_run(ctx, rec, on_device, status, chain, seq_genome, n_genome, req, nullptr, nullptr);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

extern "C" int swg_gaps_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, const uint32_t* seq_genome,
                                uint32_t n_genome, swg_gaps_request* req) {
  return records_abi(ctx, rec, false, status, chain, seq_genome, n_genome, req);
}

extern "C" int swg_gaps_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, const uint32_t* seq_genome,
                                       uint32_t n_genome, swg_gaps_request* req) {
  return records_abi(ctx, rec, true, status, chain, seq_genome, n_genome, req);
}

// The gaps texts of an open PAF: records and genome map from the handle (the last-'#' map of swg_paf_breadth), rows and summary
// from ONE device call, the formatting in host/gaps_text.cpp.  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_gaps(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const uint32_t* chain, uint32_t min_size, char** rows_text,
                            uint64_t* rows_len, char** summary_text, uint64_t* summary_len) {
  if (rows_text) *rows_text = nullptr;
  if (rows_len) *rows_len = 0;
  if (summary_text) *summary_text = nullptr;
  if (summary_len) *summary_len = 0;
  if (!p || (!rows_text && !summary_text) || (rows_text && !rows_len) || (summary_text && !summary_len))
    return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_gaps: NULL argument, or neither text is asked for");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))  // (before the context is looked at)
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED, "swg_paf_gaps: the file has a value >= 2^32, its columns are rebased: gaps of 64-bit columns are not supported");
  const swg_records* rec = swg_paf_records(p);
  const uint64_t n = rec->n;
  try {
    std::vector<swg_gap_row> rows;
    std::vector<swg_gap_pair> pairs;
    std::vector<std::string> gname;
    uint64_t spectrum[2 * BINS] = {0};
    bool any = false;
    if (n && (!status || !chain)) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_gaps: NULL status or chain");
    for (uint64_t i = 0; i < n && !any; ++i) any = status[i] == SWG_ST_SCAFFOLD && chain[i] != 0;
    if (any) {
      if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_gaps: NULL context");
      swg_gaps_request req{};
      req.min_size = min_size;
      req.want = (rows_text ? SWG_GAPS_ROWS : 0u) | (summary_text ? SWG_GAPS_SUMMARY : 0u);
      req.spectrum = spectrum;
      const int rc = gaps_run(ctx, rec, false, status, chain, rec->seq_genome_last, rec->n_genome_last, &req, &rows, &pairs);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      swg_paf_stats_genome_names(p, &gname);
    }
    const std::string text[2] = {rows_text ? swg_gaps_rows_text(p, rec, rows) : std::string(),
                                 summary_text ? swg_gaps_summary_text(gname, pairs, spectrum) : std::string()};
    const bool wanted[2] = {rows_text != nullptr, summary_text != nullptr};
    char* out[2] = {nullptr, nullptr};
    uint64_t len[2] = {0, 0};
    SWG_TRY(texts_hand_over(text, wanted, 2, out, len));
    if (rows_text) *rows_text = out[0], *rows_len = len[0];
    if (summary_text) *summary_text = out[1], *summary_len = len[1];
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
