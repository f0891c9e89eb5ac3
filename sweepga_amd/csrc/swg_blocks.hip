// Blocks: one row per scaffold chain that a filter call kept -- where it lies on both sequences, how many
// mappings it has, their sums, and the bases of either sequence under at least one of them -- from the record columns plus the
// status and chain columns as swg_filter* writes them.  A record takes part when status != 0 and chain != 0.
//
//   blocks_max      C = the largest chain number of a record that takes part, and how many take part.
//   blocks_reduce   one pass over the records in input order, four consecutive ones per thread (16-byte loads), into a dense
//                   table of C + 1 rows indexed by chain number: per strand the span, count and first record of the SCAFFOLD
//                   records, the RESCUED count, minimum and maximum of the two sequence ids, the four sums.  Minima are kept as
//                   maxima of the complement, so a zeroed table is the neutral element of every field and a zero never needs an
//                   atomic.  A thread folds its records of one chain; what it holds last goes along the lanes, where runs of one
//                   chain are folded towards the run's first lane: one atomic per (run, quantity that is not zero).  The flush
//                   that finds a row's record count at zero counts the row: the number of blocks is known after this pass.
//   blocks_keys     per axis: key = chain << 32 | start, value = record; records that take no part get the chain C + 1.
//   (sort)          swg_radix_sort_pairs over the 32 + bits(C + 1) key bits.
//   blocks_gather   swg_union_tiles.h: the ends in sorted order and the tile maxima of chain << 32 | end.
//   (scan)          swg_inclusive_max_scan_u64 over the tile maxima: the carry across work-groups, with no wait inside a launch.
//   blocks_union    the tile again: running maximum before each record (running_max_before; 0 when it belongs to an earlier
//                   chain), contribution =
//                   max(0, end - max(start, running maximum)), folded like blocks_reduce -- the sorted order puts a chain's
//                   records side by side -- and added to the row's cover of the axis.
//   blocks_collect  the occupied rows as swg_block (the strand is chosen here); a chain over two sequence pairs or without a
//                   SCAFFOLD record is reported.  The host orders the rows by chain number.
//
// Device memory, from the context's arena: 28 bytes per record (two 8-byte key buffers, two 4-byte value buffers, one 4-byte
// buffer of ends; both axes use the same ones) plus the radix sort's histograms, 120 bytes per chain NUMBER (C + 1 rows of 18
// 32-bit and 6 64-bit words) and 104 bytes per block.  The host seam stages 9 columns and 2 bytes per record: 38 bytes more.
// Integer atomics only (add and max); no floating point; the result does not depend on record order or grid shape
// (first_record is the smallest index, whatever the order).
#include <algorithm>
#include <new>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;   // TB, WAVES, run_end, run_sum, wave_place, reserve_first
using namespace swg_union_tiles;  // the tile of the sorted order, its first pass and the running maximum

// a row's 32-bit words; *_NMIN hold the complement of a minimum
enum { W_QS_NMIN = 0, W_QE_MAX, W_TS_NMIN, W_TE_MAX, W_COUNT, W_FIRST_NMIN, W_STRAND = 6 /* words per strand */,
       W_RESCUED = 12, W_QID_NMIN, W_QID_MAX, W_TID_NMIN, W_TID_MAX, W_RECORDS, W32 };
enum { S_MATCHES = 0, S_BLOCK_LEN, S_Q_BASES, S_T_BASES, S_FOLDED /* folded by blocks_reduce */, S_Q_COVER = 4, S_T_COVER, W64 };
enum { D_MAX_CHAIN = 0, D_TAKING, D_BAD_ID, D_BLOCKS, D_LISTED, D_TWO_PAIRS, D_NO_SCAFFOLD, D_TOTAL };
static_assert(W32 == 18 && W64 == 6, "the header comment and include/sweepga_gpu.h state 120 bytes per chain number");

__host__ __device__ constexpr bool word_adds(int i) { return i == W_COUNT || i == W_STRAND + W_COUNT || i == W_RESCUED || i == W_RECORDS; }

struct BlockTable {
  uint32_t* w;            // [C + 1][W32]
  unsigned long long* s;  // [C + 1][W64]
  uint32_t C;
};

// what a thread, then a run of lanes, holds of one chain (chain 0: nothing)
struct Acc {
  uint32_t chain;
  uint32_t w[W32];
  unsigned long long s[S_FOLDED];
};

__device__ __forceinline__ void acc_clear(Acc& a) {
  a.chain = 0;
#pragma unroll
  for (int i = 0; i < W32; ++i) a.w[i] = 0;
#pragma unroll
  for (int i = 0; i < S_FOLDED; ++i) a.s[i] = 0;
}

struct Record {
  uint32_t q_id, t_id, qs, qe, ts, te, matches, block_len, chain, index;
  uint8_t strand, status;
};

template <int ST>
__device__ __forceinline__ void acc_member(Acc& a, const Record& r) {  // a SCAFFOLD record of strand ST
  a.w[ST * W_STRAND + W_QS_NMIN] = max(a.w[ST * W_STRAND + W_QS_NMIN], ~r.qs);
  a.w[ST * W_STRAND + W_QE_MAX] = max(a.w[ST * W_STRAND + W_QE_MAX], r.qe);
  a.w[ST * W_STRAND + W_TS_NMIN] = max(a.w[ST * W_STRAND + W_TS_NMIN], ~r.ts);
  a.w[ST * W_STRAND + W_TE_MAX] = max(a.w[ST * W_STRAND + W_TE_MAX], r.te);
  a.w[ST * W_STRAND + W_COUNT] += 1;
  a.w[ST * W_STRAND + W_FIRST_NMIN] = max(a.w[ST * W_STRAND + W_FIRST_NMIN], ~r.index);
}

__device__ __forceinline__ void acc_record(Acc& a, const Record& r) {
  a.chain = r.chain;
  if (r.status == SWG_ST_SCAFFOLD) {  // (two instances: no dynamic index into the registers)
    if (r.strand == 0)
      acc_member<0>(a, r);
    else
      acc_member<1>(a, r);
  }
  a.w[W_RESCUED] += r.status == SWG_ST_RESCUED;
  a.w[W_QID_NMIN] = max(a.w[W_QID_NMIN], ~r.q_id);
  a.w[W_QID_MAX] = max(a.w[W_QID_MAX], r.q_id);
  a.w[W_TID_NMIN] = max(a.w[W_TID_NMIN], ~r.t_id);
  a.w[W_TID_MAX] = max(a.w[W_TID_MAX], r.t_id);
  a.w[W_RECORDS] += 1;
  a.s[S_MATCHES] += r.matches;
  a.s[S_BLOCK_LEN] += r.block_len;
  a.s[S_Q_BASES] += r.qe > r.qs ? r.qe - r.qs : 0u;
  a.s[S_T_BASES] += r.te > r.ts ? r.te - r.ts : 0u;
}

// one atomic per quantity that is not zero (a zero changes neither a sum nor a maximum over unsigned values)
__device__ __forceinline__ void acc_flush(const BlockTable& T, const Acc& a, unsigned long long* scalars) {
  if (a.chain == 0) return;
  uint32_t* row = T.w + (size_t)a.chain * W32;
#pragma unroll
  for (int i = 0; i < W32; ++i) {
    if (i == W_RECORDS || a.w[i] == 0) continue;
    if (word_adds(i))
      atomicAdd(&row[i], a.w[i]);
    else
      atomicMax(&row[i], a.w[i]);
  }
  if (atomicAdd(&row[W_RECORDS], a.w[W_RECORDS]) == 0) atomicAdd(&scalars[D_BLOCKS], 1ull);  // (a.w[W_RECORDS] >= 1: one flush finds 0)
  unsigned long long* sums = T.s + (size_t)a.chain * W64;
#pragma unroll
  for (int i = 0; i < S_FOLDED; ++i)
    if (a.s[i]) atomicAdd(&sums[i], a.s[i]);
}

// runs of one chain along the lanes, folded towards the run's first lane, which flushes
__device__ __forceinline__ void acc_fold_lanes(const BlockTable& T, Acc& a, unsigned long long* scalars) {
  if (__ballot(a.chain != 0) == 0) return;  // wavefront-uniform
  const int lane = threadIdx.x & 63;
  const uint32_t before = __shfl_up(a.chain, 1);
  const bool first_lane = lane == 0 || a.chain != before;
  const int end = run_end(__ballot(first_lane), lane);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const bool take = lane + d < end;
#pragma unroll
    for (int i = 0; i < W32; ++i) {
      const uint32_t o = __shfl_down(a.w[i], d);
      if (take) a.w[i] = word_adds(i) ? a.w[i] + o : max(a.w[i], o);
    }
#pragma unroll
    for (int i = 0; i < S_FOLDED; ++i) {
      const unsigned long long o = __shfl_down(a.s[i], d);
      if (take) a.s[i] += o;
    }
  }
  if (first_lane) acc_flush(T, a, scalars);
}

struct Cols {
  const uint32_t *q_id, *t_id, *start[2], *end[2], *matches, *block_len, *chain;
  const uint8_t *strand, *status;
};

// ---- the largest chain number ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void blocks_max_kernel(uint64_t n, const uint32_t* __restrict__ chain, const uint8_t* __restrict__ status,
                                                        unsigned long long* __restrict__ scalars) {
  uint32_t m = 0;
  unsigned long long taking = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TB) {
    const uint32_t c = status[i] != 0 ? chain[i] : 0u;
    m = max(m, c);
    taking += c != 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor(m, d));
  taking = wave_sum(taking);
  if ((threadIdx.x & 63) == 0) {
    if (m) atomicMax(&scalars[D_MAX_CHAIN], (unsigned long long)m);
    if (taking) atomicAdd(&scalars[D_TAKING], taking);
  }
}

// ---- the reduce pass -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load4(const uint32_t* __restrict__ col, uint64_t n, uint64_t p0, bool vec, uint32_t (&v)[ITEMS]) {
  if (vec) {
    const uint4 w = *reinterpret_cast<const uint4*>(col + p0);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) v[j] = p0 + j < n ? col[p0 + j] : 0u;
  }
}
__device__ __forceinline__ void load4(const uint8_t* __restrict__ col, uint64_t n, uint64_t p0, bool vec, uint8_t (&v)[ITEMS]) {
  if (vec) {
    const uchar4 w = *reinterpret_cast<const uchar4*>(col + p0);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) v[j] = p0 + j < n ? col[p0 + j] : (uint8_t)0;
  }
}

// `aligned`: every column starts on a 16-byte boundary (the byte columns on a 4-byte one), so that a thread's four records are
// one load per column
__global__ __launch_bounds__(TB) void blocks_reduce_kernel(uint64_t n, Cols c, uint32_t n_seq, bool aligned, BlockTable T,
                                                           unsigned long long* __restrict__ scalars) {
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  const bool vec = aligned && p0 + ITEMS <= n;
  uint32_t chain[ITEMS], q_id[ITEMS], t_id[ITEMS], qs[ITEMS], qe[ITEMS], ts[ITEMS], te[ITEMS], matches[ITEMS], block_len[ITEMS];
  uint8_t status[ITEMS], strand[ITEMS];
  load4(c.chain, n, p0, vec, chain);
  load4(c.status, n, p0, vec, status);
  load4(c.strand, n, p0, vec, strand);
  load4(c.q_id, n, p0, vec, q_id);
  load4(c.t_id, n, p0, vec, t_id);
  load4(c.start[0], n, p0, vec, qs);
  load4(c.end[0], n, p0, vec, qe);
  load4(c.start[1], n, p0, vec, ts);
  load4(c.end[1], n, p0, vec, te);
  load4(c.matches, n, p0, vec, matches);
  load4(c.block_len, n, p0, vec, block_len);
  Acc a;
  acc_clear(a);
  bool bad = false;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (p0 + j >= n) continue;
    bad |= q_id[j] >= n_seq || t_id[j] >= n_seq;
    if (status[j] == 0 || chain[j] == 0 || chain[j] > T.C) continue;  // (chain <= C by blocks_max; the test keeps every index inside the table)
    if (a.chain != chain[j]) {  // (a record that takes no part does not end a thread's run)
      acc_flush(T, a, scalars);
      acc_clear(a);
    }
    acc_record(a, Record{q_id[j], t_id[j], qs[j], qe[j], ts[j], te[j], matches[j], block_len[j], chain[j], (uint32_t)(p0 + j), strand[j], status[j]});
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&scalars[D_BAD_ID], 1ull);
  acc_fold_lanes(T, a, scalars);
}

// ---- covers --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void blocks_keys_kernel(uint64_t n, const uint32_t* __restrict__ chain, const uint8_t* __restrict__ status,
                                                         const uint32_t* __restrict__ start, uint32_t C, uint64_t* __restrict__ keys,
                                                         uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = status[i] != 0 ? chain[i] : 0u;
  keys[i] = c != 0 && c <= C ? ((uint64_t)c << 32) | start[i] : (uint64_t)(C + 1) << 32;
  vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(TB) void blocks_gather_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ end_col, uint32_t sentinel,
                                                           uint32_t* __restrict__ ends, unsigned long long* __restrict__ tile_max, uint64_t ntiles) {
  gather_tile<false>(n, keys, vals, end_col, sentinel, ends, tile_max, ntiles, nullptr);
}

// cover: S_Q_COVER or S_T_COVER
__global__ __launch_bounds__(TB) void blocks_union_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry,
                                                          uint32_t sentinel, BlockTable T, int cover) {
  __shared__ unsigned long long l_wave[1][WAVES];
  const int lane = threadIdx.x & 63;
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint64_t k[ITEMS];
  uint32_t v[ITEMS], e[ITEMS];
  load_tile(keys, vals, n, p0, k, v);
  load_ends(ends, n, p0, e);
  bool counted[ITEMS];
  unsigned long long mine[1] = {0};
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    counted[j] = p0 + j < n && (uint32_t)(k[j] >> 32) != sentinel;
    if (counted[j]) mine[0] = max64(mine[0], (k[j] & 0xffffffff00000000ull) | e[j]);
  }
  unsigned long long front[1];
  running_max_before<1>(mine, l_wave, carry, 0, 1u, front);  // (one set: no second row of tile maxima, ntiles is not read)
  unsigned long long r = front[0];
  // contributions, folded along the thread and then along the lanes
  uint32_t run_chain = 0;
  unsigned long long run[1] = {0};
  unsigned long long* covers = T.s + cover;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (!counted[j]) continue;
    const uint32_t c = (uint32_t)(k[j] >> 32), start = (uint32_t)k[j];
    const uint32_t m = (uint32_t)(r >> 32) == c ? (uint32_t)r : 0u;
    const uint32_t lo = start > m ? start : m;
    const uint32_t add = e[j] > lo ? e[j] - lo : 0u;
    r = max64(r, (k[j] & 0xffffffff00000000ull) | e[j]);
    if (c != run_chain) {
      if (run[0]) atomicAdd(&covers[(size_t)run_chain * W64], run[0]);
      run_chain = c, run[0] = 0;
    }
    run[0] += add;
  }
  if (__ballot(run_chain != 0) == 0) return;  // wavefront-uniform, behind the barrier
  const uint32_t before = __shfl_up(run_chain, 1);
  const bool first_lane = lane == 0 || run_chain != before;
  run_sum(run, lane, run_end(__ballot(first_lane), lane));
  if (first_lane && run_chain != 0 && run[0]) atomicAdd(&covers[(size_t)run_chain * W64], run[0]);
}

// ---- the occupied rows -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void blocks_collect_kernel(BlockTable T, swg_block* __restrict__ out, uint64_t cap,
                                                            unsigned long long* __restrict__ scalars) {
  const uint64_t c = (uint64_t)blockIdx.x * TB + threadIdx.x + 1;
  const bool in = c <= T.C;
  const uint32_t* w = T.w + (in ? c : 0) * W32;
  const bool have = in && w[W_RECORDS] != 0;
  const unsigned long long at = wave_place(__ballot(have), &scalars[D_LISTED]);
  if (!have) return;
  if (w[W_QID_MAX] != ~w[W_QID_NMIN] || w[W_TID_MAX] != ~w[W_TID_NMIN]) atomicMax(&scalars[D_TWO_PAIRS], (unsigned long long)c);
  if (w[W_COUNT] + w[W_STRAND + W_COUNT] == 0) atomicMax(&scalars[D_NO_SCAFFOLD], (unsigned long long)c);
  if (at >= cap) return;
  const int st = w[W_COUNT] != 0 ? 0 : 1;  // '+' if any SCAFFOLD record is '+': its '-' ones are the captured inversions
  const uint32_t* core = w + st * W_STRAND;
  const unsigned long long* s = T.s + c * W64;
  swg_block b;
  b.chain = (uint32_t)c;
  b.q_id = w[W_QID_MAX];
  b.t_id = w[W_TID_MAX];
  b.strand = (uint32_t)st;
  b.q_start = ~core[W_QS_NMIN];
  b.q_end = core[W_QE_MAX];
  b.t_start = ~core[W_TS_NMIN];
  b.t_end = core[W_TE_MAX];
  b.n_core = core[W_COUNT];
  b.n_inverted = st == 0 ? w[W_STRAND + W_COUNT] : 0u;
  b.n_rescued = w[W_RESCUED];
  b.reserved = 0;
  b.matches = s[S_MATCHES];
  b.block_len = s[S_BLOCK_LEN];
  b.q_bases = s[S_Q_BASES];
  b.t_bases = s[S_T_BASES];
  b.q_cover = s[S_Q_COVER];
  b.t_cover = s[S_T_COVER];
  b.first_record = (uint32_t)~core[W_FIRST_NMIN];
  out[at] = b;
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// inside an arena frame
int blocks_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const Cols& d, swg_blocks_result* res) {
  hipStream_t st = ctx->stream;
  const uint64_t ntiles = (n + TILE - 1) / TILE;
  const unsigned grid_n = (unsigned)((n + TB - 1) / TB), grid_t = (unsigned)ntiles;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  SWG_LAUNCH(ctx, "blocks_max", blocks_max_kernel<<<grid_for(ctx, n), TB, 0, st>>>(n, d.chain, d.status, scalars));
  SWG_KERNEL_CHECK(ctx);
  uint64_t h[D_TOTAL];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 2));
  if (h[D_MAX_CHAIN] == 0) return SWG_OK;  // no chain: no block
  if (h[D_MAX_CHAIN] >= 0xffffffffull) return swg_set_error(ctx, SWG_ERR_RANGE, "blocks: chain number 2^32 - 1 (one past the last chain has to fit 32 bits)");
  BlockTable T{};
  T.C = (uint32_t)h[D_MAX_CHAIN];
  const size_t rows = (size_t)T.C + 1;
  T.w = swg_alloc<uint32_t>(ctx, rows * W32);
  T.s = swg_alloc<unsigned long long>(ctx, rows * W64);
  uint64_t* keys = swg_alloc<uint64_t>(ctx, n);
  uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n);
  uint32_t* vals = swg_alloc<uint32_t>(ctx, n);
  uint32_t* vals_alt = swg_alloc<uint32_t>(ctx, n);
  uint32_t* ends = swg_alloc<uint32_t>(ctx, n);
  unsigned long long* tile_max = swg_alloc<unsigned long long>(ctx, ntiles);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(T.w, 0, rows * W32 * sizeof(uint32_t), st));
  SWG_HIP(ctx, hipMemsetAsync(T.s, 0, rows * W64 * sizeof(unsigned long long), st));
  bool aligned = aligned_to(d.strand, 4) && aligned_to(d.status, 4);
  for (const uint32_t* p : {d.q_id, d.t_id, d.start[0], d.start[1], d.end[0], d.end[1], d.matches, d.block_len, d.chain}) aligned = aligned && aligned_to(p, 16);
  SWG_LAUNCH(ctx, "blocks_reduce", blocks_reduce_kernel<<<grid_t, TB, 0, st>>>(n, d, n_seq, aligned, T, scalars));
  SWG_KERNEL_CHECK(ctx);
  const uint32_t sentinel = T.C + 1;
  const int end_bit = 32 + swg_bits_for(sentinel);
  for (int axis = 0; axis < 2; ++axis) {
    SWG_LAUNCH(ctx, "blocks_keys", blocks_keys_kernel<<<grid_n, TB, 0, st>>>(n, d.chain, d.status, d.start[axis], T.C, keys, vals));
    SWG_KERNEL_CHECK(ctx);
    {
      swg_prof_scope sort_scope(ctx, axis == 0 ? "blocks_sort_q" : "blocks_sort_t");
      SWG_TRY(swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, n, 0, end_bit));
    }
    SWG_LAUNCH(ctx, "blocks_gather", blocks_gather_kernel<<<grid_t, TB, 0, st>>>(n, keys, vals, d.end[axis], sentinel, ends, tile_max, ntiles));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max), reinterpret_cast<uint64_t*>(tile_max), ntiles));
    SWG_LAUNCH(ctx, "blocks_union", blocks_union_kernel<<<grid_t, TB, 0, st>>>(n, keys, vals, ends, tile_max, sentinel, T, axis == 0 ? S_Q_COVER : S_T_COVER));
    SWG_KERNEL_CHECK(ctx);
  }
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  if (h[D_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "blocks: a sequence id >= n_seq");
  const uint64_t n_blocks = h[D_BLOCKS];
  if (n_blocks == 0 || n_blocks > h[D_TAKING])
    return swg_set_error(ctx, SWG_ERR_HIP, "blocks: internal: %llu blocks from %llu records", (unsigned long long)n_blocks, (unsigned long long)h[D_TAKING]);
  swg_block* list = swg_alloc<swg_block>(ctx, n_blocks);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "blocks_collect", blocks_collect_kernel<<<(unsigned)(((uint64_t)T.C + TB - 1) / TB), TB, 0, st>>>(T, list, n_blocks, scalars));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  if (h[D_TWO_PAIRS])
    return swg_set_error(ctx, SWG_ERR_INVALID, "blocks: the records of chain %llu name more than one (q_id, t_id) pair", (unsigned long long)h[D_TWO_PAIRS]);
  if (h[D_NO_SCAFFOLD])
    return swg_set_error(ctx, SWG_ERR_INVALID, "blocks: chain %llu has no record with status SWG_ST_SCAFFOLD", (unsigned long long)h[D_NO_SCAFFOLD]);
  if (h[D_LISTED] != n_blocks)
    return swg_set_error(ctx, SWG_ERR_HIP, "blocks: internal: %llu rows listed, %llu counted", (unsigned long long)h[D_LISTED], (unsigned long long)n_blocks);
  res->blocks.resize(n_blocks);
  SWG_HIP(ctx, hipMemcpyAsync(res->blocks.data(), list, n_blocks * sizeof(swg_block), hipMemcpyDeviceToHost, st));
  SWG_HIP(ctx, hipStreamSynchronize(st));
  std::sort(res->blocks.begin(), res->blocks.end(), [](const swg_block& a, const swg_block& b) { return a.chain < b.chain; });
  return SWG_OK;
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const uint32_t* chain, swg_block_table* table) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!table) return swg_set_error(ctx, SWG_ERR_INVALID, "blocks: NULL table");
  try {
    swg_blocks_result r;
    SWG_TRY(swg_blocks_run(ctx, rec, on_device, status, chain, &r));
    table->n_blocks = r.blocks.size();
    if (table->blocks && table->n_blocks <= table->block_capacity) std::copy(r.blocks.begin(), r.blocks.end(), table->blocks);
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

int swg_blocks_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const uint32_t* chain, swg_blocks_result* res) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !res) return swg_set_error(ctx, SWG_ERR_INVALID, "blocks: NULL records");
  res->blocks.clear();
  const uint64_t n = rec->n;
  if (n == 0) return SWG_OK;
  if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand || !rec->matches || !rec->block_len ||
      !status || !chain)
    return swg_set_error(ctx, SWG_ERR_INVALID, "blocks: NULL column (q_id, t_id, the four coordinates, strand, matches, block_len, status and chain are read)");
  if (rec->n_seq == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "blocks: records without sequences");
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "blocks: 2^31 records or more in one call");
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 72 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    Cols d{rec->q_id, rec->t_id, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->matches, rec->block_len, chain, rec->strand, status};
    if (!on_device) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&d.q_id, &d.t_id, &d.start[0], &d.start[1], &d.end[0], &d.end[1], &d.matches, &d.block_len, &d.chain}) s.add(col, n);
      s.add(&d.strand, n);
      s.add(&d.status, n);
      SWG_TRY(s.run());
    }
    return blocks_device(ctx, n, rec->n_seq, d, res);
  });
}

extern "C" int swg_blocks_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, swg_block_table* table) {
  return records_abi(ctx, rec, false, status, chain, table);
}

extern "C" int swg_blocks_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const uint32_t* chain, swg_block_table* table) {
  return records_abi(ctx, rec, true, status, chain, table);
}

// The blocks of an open PAF as PAF text: records from the handle, the table from the device, names and lengths from the line
// of each block's first record (host/paf_io.cpp).  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_blocks(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const uint32_t* chain, char** out_text, uint64_t* out_len) {
  if (out_text) *out_text = nullptr;
  if (out_len) *out_len = 0;
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_blocks: NULL argument");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED, "swg_paf_blocks: the file has a value >= 2^32, its columns are rebased: blocks of 64-bit columns are not supported");
  const swg_records* rec = swg_paf_records(p);
  const uint64_t n = rec->n;
  try {
    swg_blocks_result r;
    bool any = false;
    if (n && (!status || !chain)) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_blocks: NULL status or chain");
    for (uint64_t i = 0; i < n && !any; ++i) any = status[i] != 0 && chain[i] != 0;
    if (any) {
      if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_blocks: NULL context");
      const int rc = swg_blocks_run(ctx, rec, false, status, chain, &r);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    }
    return swg_paf_blocks_text(p, r.blocks, out_text, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
