// Mosaic: the best mapping at every base.  On one axis (0 = query, 1 = target) a record lies on a sequence
// over [start, end); it counts by breadth's rule (the genomes of its two sequences differ, non-zero length) and belongs to the set
// (ALL, or KEPT = status != 0).  P(r) = weight[r] << 32 | (0xffffffff - r): the heavier record wins, among equals the lower index.
// winner(s, x) = the record of the set on s with start <= x < end and maximal P.  The rows -- maximal stretches of one winner,
// ordered by (sequence, start) -- and the share: bases of genome g's sequences won by records whose other sequence is of genome h.
//
// The union walk of swg_union_tiles.h keeps one running maximum of ends; this needs the maximum over all intervals that stab a
// point.  It is a range-maximum update with point queries over the distinct boundaries, in two levels of sparse tables:
//
//   mosaic_keys        record r of the set: (seq << 32 | start, r) at 2 r and (seq << 32 | end, r | END_FLAG) at 2 r + 1; every
//                      other record: the sentinel key n_seq << 32 twice.  Ids are checked as in sharing_keys.
//   (sort)             swg_radix_sort_pairs over the 2n entries, 32 + bits(n_seq) key bits
//   mosaic_flags       flag[p] = key[p] differs from key[p - 1] (u32); (scan) swg_exclusive_scan_u32 in place: B distinct
//                      boundaries, read back with the bad-id bit
//   mosaic_slots       slot[p] = flags in front of p, + flag[p] - 1; the first entry of a slot writes bound[slot] = key and
//                      first[slot] = p (first[B] = 2n); every entry scatters its slot to a[r] (begin) or b[r] (end).  Record r covers
//                      the slots [a[r], b[r]); slot i stands for [bound[i], bound[i + 1]).  Records outside the set have a == b.
//   mosaic_coarse      slots are cut into tiles of T.  One thread per record: the whole tiles [ceil(a / T), floor(b / T)), c of
//                      them, k = floor(log2 c): atomicMax of P into tbl[k][first] and tbl[k][last + 1 - 2^k] (64-bit, global).
//                      Equal targets in neighbouring lanes are reduced in the lanes first.
//   mosaic_push        one launch per level k, top down: tbl[k-1][j] = max(tbl[k-1][j], tbl[k][j], tbl[k][j - 2^(k-1)]) -- the
//                      gather form of the push-down, no atomics.  Afterwards tbl[0][t] is the best record that covers tile t whole.
//   mosaic_tile        one work-group per tile.  Its entries are sorted[first[lo] .. first[hi]), walked in chunks of TB however many
//                      they are (the sentinel's entries, which put nothing, are left out).  A begin entry at local slot p puts P on
//                      [p, min(b, hi)) unless that is the whole tile (coarse has it); an end entry whose record began left of the tile puts P on [lo, p).  Same two-atomicMax decomposition,
//                      into a sparse table in LDS (log2 T levels of T entries: a partial range is shorter than T); the push-down
//                      runs there between barriers; winner[i] = max(lds[0][i - lo], tbl[0][tile]).
//   mosaic_breaks      flag[i] = winner[i] != winner[i - 1] or i == 0; (compaction) swg_flags_count / swg_flags_compact; read back
//   mosaic_open        per break: winner != 0 opens a row; (compaction) the openers; read back: the rows
//   mosaic_rows        row j = {seq, lo32(bound[opener]), lo32(bound[next break]), 0xffffffff - lo32(winner)}.  The last boundary
//                      of a sequence is covered by nothing (every end is a boundary of its own sequence), so a next break exists
//                      and lies in the same sequence.
//   mosaic_bases       sum(end - start) over the rows (rows bit)
//   mosaic_share       (share bit) per row genome(seq) and genome(other sequence of the record): end - start added to (g, h); equal
//                      keys along the lanes are summed first, then the work-group's LdsTable, one atomic per (work-group, key)
//
// No work-group waits for another inside a launch; every carry goes through the library's scans between launches.  max is
// idempotent and commutative, so neither the order of the atomics nor the order inside a group of equal keys shows in the result.
// No lane loops over a group of equal keys.  What a huge group (say 10^5 equal begins) costs instead: its entries all fall into
// one tile, so ONE work-group walks them in chunks of TB, and their LDS atomics meet at one address per level.
//
// Scratch (bytes): 48 n for the sort (2n keys and values, twice); the flags / slots live in the sort's free value buffer, a and b
// in its free key buffer.  Then 21 B + 4 for bound (8 B), winner (8 B), first (4 (B + 1)) and the break flags (B), 8 N bits(N) for
// the coarse table of N = ceil(B / T) tiles, 5 per break, 20 per row, 8 G^2 for the share; 29 n + 4 n_seq on the host seam (six
// columns, status and the weight staged).  B <= 2n + 1 and breaks <= B: with every boundary distinct about 48 n + 26 * 2n + 20 per
// row, roughly 100 n + 20 R; a context's first call reserves 112 n.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;
using swg_union_tiles::ARG_COUNTS;
using swg_union_tiles::ARG_LIMIT;
using swg_union_tiles::SegCols;

#ifndef SWG_MOSAIC_TILE_LOG
#define SWG_MOSAIC_TILE_LOG 9  // T = 512: nine levels of 512 u64 = 36,864 bytes of LDS, four work-groups per CU
#endif
constexpr int TILE_LOG = SWG_MOSAIC_TILE_LOG;
constexpr int T_MAX = 1 << TILE_LOG;
static_assert(TILE_LOG >= 8 && TILE_LOG <= 10, "T is 256, 512 or 1024");
constexpr uint32_t END_FLAG = 0x80000000u;
constexpr unsigned long long NO_SLOT = ~0ull;
constexpr uint32_t MAX_SHARE_GENOMES = 4096;
enum { D_BAD = 0, D_BOUNDS = 1, D_BREAKS = 2, D_ROWS = 3, D_BASES = 4, D_TOTAL = 5 };
using ShareTable = PairTable<1, false>;  // dense: slot = g * G + h

// SWG_MOSAIC_TILE (environment, read once): a smaller tile, a power of two from 2 to T, for tests that need the tile seams on
// small inputs.  Anything else is ignored.
int tile_log() {
  static const int v = [] {
    const char* e = std::getenv("SWG_MOSAIC_TILE");
    if (e && *e) {
      const long t = std::strtol(e, nullptr, 10);
      for (int k = 1; k <= TILE_LOG; ++k)
        if (t == (1L << k)) return k;
    }
    return TILE_LOG;
  }();
  return v;
}

struct Weight {           // the weight of record r: w[r], or without w the record's length on the axis
  const uint32_t* w;
  const uint32_t *start, *end;
  __device__ __forceinline__ unsigned long long prio(uint32_t r) const {
    const uint32_t v = w ? w[r] : end[r] - start[r];
    return ((unsigned long long)v << 32) | (0xffffffffu - r);
  }
};

__global__ __launch_bounds__(TB) void mosaic_keys_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                         const uint32_t* __restrict__ start, const uint32_t* __restrict__ end,
                                                         const uint8_t* __restrict__ status, const uint32_t* __restrict__ seq_genome, uint32_t n_seq,
                                                         uint32_t G, uint32_t axis, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                         unsigned long long* __restrict__ scalars) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = q_id[i], t = t_id[i];
  const uint32_t gq = q < n_seq ? seq_genome[q] : NONE32, gt = t < n_seq ? seq_genome[t] : NONE32;
  uint64_t key_b = (uint64_t)n_seq << 32, key_e = key_b;
  if (gq >= G || gt >= G) {
    atomicOr(&scalars[D_BAD], 1ull);
  } else if (gq != gt && (!status || status[i] != 0)) {
    const uint32_t s = axis ? t : q, from = start[i], to = end[i];
    if (from < to) key_b = ((uint64_t)s << 32) | from, key_e = ((uint64_t)s << 32) | to;
  }
  keys[2 * i] = key_b, vals[2 * i] = (uint32_t)i;
  keys[2 * i + 1] = key_e, vals[2 * i + 1] = (uint32_t)i | END_FLAG;
}

__global__ __launch_bounds__(TB) void mosaic_flags_kernel(const uint64_t* __restrict__ keys, uint64_t n2, uint32_t* __restrict__ flag) {
  const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (p >= n2) return;
  flag[p] = p == 0 || keys[p - 1] != keys[p];
}

// slot[p]: in, the flags in front of p; out, p's slot
__global__ __launch_bounds__(TB) void mosaic_slots_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t n2, uint64_t B,
                                                          uint32_t* __restrict__ slot, uint64_t* __restrict__ bound, uint32_t* __restrict__ first,
                                                          uint32_t* __restrict__ a, uint32_t* __restrict__ b) {
  const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (p >= n2) return;
  const uint64_t key = keys[p];
  const bool head = p == 0 || keys[p - 1] != key;
  const uint32_t s = slot[p] + (head ? 1u : 0u) - 1u;
  slot[p] = s;
  if (head && s < B) bound[s] = key, first[s] = (uint32_t)p;
  if (p == 0) first[B] = (uint32_t)n2;
  const uint32_t v = vals[p];
  (v & END_FLAG ? b : a)[v & ~END_FLAG] = s;
}

// atomicMax of p into tbl[at] for every lane with a slot (NO_SLOT = none); runs of one slot along the lanes are reduced towards
// their first lane first.  Called by whole wavefronts.
__device__ __forceinline__ void run_max_put(unsigned long long* tbl, unsigned long long at, unsigned long long p) {
  const int lane = threadIdx.x & 63;
  const unsigned long long left = __shfl_up(at, 1);
  const bool first_lane = lane == 0 || at != left;
  const int end = run_end(__ballot(first_lane), lane);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_down(p, d);
    if (lane + d < end && o > p) p = o;
  }
  if (first_lane && at != NO_SLOT) atomicMax(&tbl[at], p);
}

// P on the positions [from, to) of a sparse table with `stride` entries per level: level k = floor(log2(to - from)), at `from`
// and at to - 2^k.  The two stretches of 2^k lie inside [from, to) and cover it.  from >= to: nothing.  Whole wavefronts.
__device__ __forceinline__ void range_put(unsigned long long* tbl, uint64_t stride, uint32_t from, uint32_t to, unsigned long long p) {
  unsigned long long at0 = NO_SLOT, at1 = NO_SLOT;
  if (from < to) {
    const int k = 31 - __builtin_clz(to - from);
    at0 = (uint64_t)k * stride + from;
    at1 = (uint64_t)k * stride + (to - (1u << k));
  }
  run_max_put(tbl, at0, p);
  run_max_put(tbl, at1, p);
}

__global__ __launch_bounds__(TB) void mosaic_coarse_kernel(uint64_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, Weight W,
                                                           int tile_log, uint64_t n_tiles, unsigned long long* __restrict__ tbl) {
  const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;  // (no early return: whole wavefronts vote)
  uint32_t from = 0, to = 0;
  unsigned long long p = 0;
  if (r < n) {
    const uint32_t lo = a[r], hi = b[r];
    if (lo < hi) {
      from = (uint32_t)(((uint64_t)lo + (1u << tile_log) - 1) >> tile_log);
      to = hi >> tile_log;
      if (from < to) p = W.prio((uint32_t)r);
    }
  }
  range_put(tbl, n_tiles, from, to, p);
}

// level k -> level k - 1 (upper = tbl[k], lower = tbl[k - 1], half = 2^(k-1)): an entry of level k stands for two of level k - 1
__global__ __launch_bounds__(TB) void mosaic_push_kernel(const unsigned long long* __restrict__ upper, unsigned long long* __restrict__ lower,
                                                         uint64_t n_tiles, uint64_t half) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= n_tiles) return;
  unsigned long long v = lower[j];
  v = max(v, upper[j]);
  if (j >= half) v = max(v, upper[j - half]);
  lower[j] = v;
}

__global__ __launch_bounds__(TB) void mosaic_tile_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ slot,
                                                         const uint32_t* __restrict__ first, const uint64_t* __restrict__ bound,
                                                         const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, Weight W,
                                                         int tile_log, uint64_t B, uint32_t n_seq,
                                                         const unsigned long long* __restrict__ coarse, unsigned long long* __restrict__ winner) {
  __shared__ unsigned long long l_tbl[TILE_LOG * T_MAX];  // level k at k * T_MAX
  const uint32_t T = 1u << tile_log;
  const uint64_t lo = (uint64_t)blockIdx.x << tile_log, hi = min(lo + T, B);
  for (int k = 0; k < tile_log; ++k)
    for (uint32_t i = threadIdx.x; i < T; i += TB) l_tbl[k * T_MAX + i] = 0;
  __syncthreads();
  // (the sentinel's slot, the last one when there is one, holds both entries of every record outside the set -- most of a KEPT
  // call's entries -- and none of them puts anything: the walk ends in front of it)
  const uint64_t e0 = first[lo], e1 = hi == B && (uint32_t)(bound[B - 1] >> 32) == n_seq ? first[B - 1] : first[hi];
  for (uint64_t base = e0; base < e1; base += TB) {  // (uniform: whole wavefronts vote)
    const uint64_t p = base + threadIdx.x;
    uint32_t from = 0, to = 0;
    unsigned long long pr = 0;
    if (p < e1) {
      const uint32_t v = vals[p], r = v & ~END_FLAG, at = (uint32_t)(slot[p] - lo);
      if (v & END_FLAG) {
        if (a[r] < lo) to = at;  // the record's last, partial tile: [lo, its end)
      } else {
        from = at, to = (uint32_t)(min((uint64_t)b[r], hi) - lo);
        if (from == 0 && to == T) to = 0;  // the whole tile: mosaic_coarse has it
      }
      if (from < to) pr = W.prio(r);
    }
    range_put(l_tbl, T_MAX, from, to, pr);
  }
  __syncthreads();
  for (int k = tile_log - 1; k >= 1; --k) {
    const uint32_t half = 1u << (k - 1);
    for (uint32_t j = threadIdx.x; j < T; j += TB) {
      unsigned long long v = max(l_tbl[(k - 1) * T_MAX + j], l_tbl[k * T_MAX + j]);
      if (j >= half) v = max(v, l_tbl[k * T_MAX + j - half]);
      l_tbl[(k - 1) * T_MAX + j] = v;
    }
    __syncthreads();
  }
  const unsigned long long whole = coarse[blockIdx.x];
  for (uint32_t i = threadIdx.x; lo + i < hi; i += TB) winner[lo + i] = max(l_tbl[i], whole);
}

__global__ __launch_bounds__(TB) void mosaic_breaks_kernel(const unsigned long long* __restrict__ winner, uint64_t B, uint8_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= B) return;
  flag[i] = i == 0 || winner[i] != winner[i - 1];
}

__global__ __launch_bounds__(TB) void mosaic_open_kernel(const uint32_t* __restrict__ breaks, uint64_t n_breaks, const unsigned long long* __restrict__ winner,
                                                         uint8_t* __restrict__ flag) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= n_breaks) return;
  flag[j] = winner[breaks[j]] != 0;
}

__global__ __launch_bounds__(TB) void mosaic_rows_kernel(const uint32_t* __restrict__ openers, uint64_t n_rows, const uint32_t* __restrict__ breaks,
                                                         uint64_t n_breaks, const uint64_t* __restrict__ bound,
                                                         const unsigned long long* __restrict__ winner, swg_mosaic_row* __restrict__ rows) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= n_rows) return;
  const uint64_t i = openers[j];
  const uint32_t at = breaks[i];
  const uint64_t key = bound[at];
  // (always i + 1 < n_breaks: nothing covers a sequence's last boundary, so an opener is never the last break)
  const uint32_t end = i + 1 < n_breaks ? (uint32_t)bound[breaks[i + 1]] : (uint32_t)key;
  rows[j] = swg_mosaic_row{(uint32_t)(key >> 32), (uint32_t)key, end, 0xffffffffu - (uint32_t)winner[at]};
}

__global__ __launch_bounds__(TB) void mosaic_bases_kernel(const swg_mosaic_row* __restrict__ rows, uint64_t n_rows, unsigned long long* __restrict__ sum) {
  swg_union_tiles::bases_sum(rows, n_rows, sum);
}

__global__ __launch_bounds__(TB) void mosaic_share_kernel(const swg_mosaic_row* __restrict__ rows, uint64_t n_rows, const uint32_t* __restrict__ other_id,
                                                          const uint32_t* __restrict__ seq_genome, uint32_t G, ShareTable T) {
  __shared__ LdsTable<1, false> l_table;
  l_table.clear();
  __syncthreads();
  for (uint64_t base = (uint64_t)blockIdx.x * TB; base < n_rows; base += (uint64_t)gridDim.x * TB) {  // (uniform: whole wavefronts vote)
    const uint64_t x = base + threadIdx.x;
    unsigned long long key = EMPTY;
    unsigned long long v[1] = {0};
    if (x < n_rows) {
      const swg_mosaic_row r = rows[x];
      key = (unsigned long long)seq_genome[r.seq] * G + seq_genome[other_id[r.record]];  // (both ids passed mosaic_keys' check)
      v[0] = r.end - r.start;
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long left = __shfl_up(key, 1);
    const bool first_lane = lane == 0 || key != left;
    run_sum(v, lane, run_end(__ballot(first_lane), lane));
    if (first_lane && key != EMPTY && v[0]) {
      if (!l_table.add(key, v)) table_add<1, false>(T, key, v, 0);  // more keys in this work-group's share than the LDS table takes
    }
  }
  __syncthreads();
  l_table.flush(T, 0);
}

// inside an arena frame.  weight: on the device, nullptr = the length on the axis.  vec: receives the rows instead of req->rows.
int mosaic_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const SegCols& d, const uint32_t* weight, swg_mosaic_request* req,
                  std::vector<swg_mosaic_row>* vec) {
  hipStream_t st = ctx->stream;
  const uint32_t axis = req->axis;
  const bool want_rows = (req->want & SWG_MOSAIC_ROWS) != 0, want_share = (req->want & SWG_MOSAIC_SHARE) != 0;
  const uint64_t n2 = 2 * n;
  const int tl = tile_log();
  const Weight W{weight, d.start[axis], d.end[axis]};
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  uint64_t* keys = swg_alloc<uint64_t>(ctx, n2);
  uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n2);
  uint32_t* vals = swg_alloc<uint32_t>(ctx, n2);
  uint32_t* vals_alt = swg_alloc<uint32_t>(ctx, n2);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  const unsigned grid_n = (unsigned)((n + TB - 1) / TB), grid_e = (unsigned)((n2 + TB - 1) / TB);
  SWG_LAUNCH(ctx, "mosaic_keys", mosaic_keys_kernel<<<grid_n, TB, 0, st>>>(n, d.q_id, d.t_id, d.start[axis], d.end[axis],
                                                                           req->set == SWG_IV_KEPT ? d.status : nullptr, d.seq_genome, n_seq, G, axis, keys,
                                                                           vals, scalars));
  SWG_KERNEL_CHECK(ctx);
  {
    swg_prof_scope sort_scope(ctx, "mosaic_sort");
    SWG_TRY(swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, n2, 0, 32 + swg_bits_for(n_seq)));
  }
  uint32_t* slot = vals_alt;  // (the sort is over: whichever buffers it left free)
  uint32_t* a = reinterpret_cast<uint32_t*>(keys_alt);
  uint32_t* b = a + n;
  SWG_LAUNCH(ctx, "mosaic_flags", mosaic_flags_kernel<<<grid_e, TB, 0, st>>>(keys, n2, slot));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_exclusive_scan_u32(ctx, slot, slot, n2, reinterpret_cast<uint64_t*>(scalars + D_BOUNDS)));
  uint64_t h[2];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 2));
  if (h[D_BAD] & 1u) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: a sequence id >= n_seq or a genome id >= n_genome");
  const uint64_t B = h[D_BOUNDS];  // (>= 1: n >= 1)
  const uint64_t n_tiles = (B + (uint64_t(1) << tl) - 1) >> tl;
  const int levels = std::max(1, swg_bits_for(n_tiles));
  uint64_t* bound = swg_alloc<uint64_t>(ctx, B);
  unsigned long long* winner = swg_alloc<unsigned long long>(ctx, B);
  unsigned long long* tbl = swg_alloc<unsigned long long>(ctx, n_tiles * levels);
  uint32_t* first = swg_alloc<uint32_t>(ctx, B + 1);
  uint8_t* flag = swg_alloc<uint8_t>(ctx, B);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(tbl, 0, n_tiles * levels * sizeof(unsigned long long), st));
  SWG_LAUNCH(ctx, "mosaic_slots", mosaic_slots_kernel<<<grid_e, TB, 0, st>>>(keys, vals, n2, B, slot, bound, first, a, b));
  SWG_KERNEL_CHECK(ctx);
  SWG_LAUNCH(ctx, "mosaic_coarse", mosaic_coarse_kernel<<<grid_n, TB, 0, st>>>(n, a, b, W, tl, n_tiles, tbl));
  SWG_KERNEL_CHECK(ctx);
  const unsigned grid_t = (unsigned)((n_tiles + TB - 1) / TB);
  for (int k = levels - 1; k >= 1; --k) {
    SWG_LAUNCH(ctx, "mosaic_push", mosaic_push_kernel<<<grid_t, TB, 0, st>>>(tbl + (uint64_t)k * n_tiles, tbl + (uint64_t)(k - 1) * n_tiles, n_tiles,
                                                                             uint64_t(1) << (k - 1)));
    SWG_KERNEL_CHECK(ctx);
  }
  SWG_LAUNCH(ctx, "mosaic_tile", mosaic_tile_kernel<<<(unsigned)n_tiles, TB, 0, st>>>(vals, slot, first, bound, a, b, W, tl, B, n_seq, tbl, winner));
  SWG_KERNEL_CHECK(ctx);
  SWG_LAUNCH(ctx, "mosaic_breaks", mosaic_breaks_kernel<<<(unsigned)((B + TB - 1) / TB), TB, 0, st>>>(winner, B, flag));
  SWG_KERNEL_CHECK(ctx);
  uint64_t n_breaks = 0, n_rows = 0;
  swg_mosaic_row* rows = nullptr;
  swg_flag_scan fs{};
  SWG_TRY(swg_flags_count(ctx, flag, B, &fs, reinterpret_cast<uint64_t*>(scalars + D_BREAKS)));
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_BREAKS), &n_breaks, 1));
  uint32_t* breaks = swg_alloc<uint32_t>(ctx, n_breaks);  // (n_breaks >= 1: slot 0 is one)
  uint8_t* o_flag = swg_alloc<uint8_t>(ctx, n_breaks);
  SWG_CHECK_ARENA(ctx);
  SWG_TRY(swg_flags_compact(ctx, fs, breaks));
  SWG_LAUNCH(ctx, "mosaic_open", mosaic_open_kernel<<<(unsigned)((n_breaks + TB - 1) / TB), TB, 0, st>>>(breaks, n_breaks, winner, o_flag));
  SWG_KERNEL_CHECK(ctx);
  swg_flag_scan fo{};
  SWG_TRY(swg_flags_count(ctx, o_flag, n_breaks, &fo, reinterpret_cast<uint64_t*>(scalars + D_ROWS)));
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_ROWS), &n_rows, 1));
  if (n_rows) {
    uint32_t* openers = swg_alloc<uint32_t>(ctx, n_rows);
    rows = swg_alloc<swg_mosaic_row>(ctx, n_rows);
    SWG_CHECK_ARENA(ctx);
    SWG_TRY(swg_flags_compact(ctx, fo, openers));
    SWG_LAUNCH(ctx, "mosaic_rows", mosaic_rows_kernel<<<(unsigned)((n_rows + TB - 1) / TB), TB, 0, st>>>(openers, n_rows, breaks, n_breaks, bound, winner, rows));
    SWG_KERNEL_CHECK(ctx);
  }
  if (want_rows) {
    uint64_t bases = 0;
    if (n_rows) {
      SWG_LAUNCH(ctx, "mosaic_bases", mosaic_bases_kernel<<<grid_for(ctx, n_rows), TB, 0, st>>>(rows, n_rows, scalars + D_BASES));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_BASES), &bases, 1));
    }
    req->n = n_rows;
    req->bases = bases;
    swg_mosaic_row* dst;
    SWG_TRY(swg_union_tiles::rows_hand_over(ctx, rows, n_rows, vec, req->rows, req->capacity, &dst));
  }
  if (want_share && n_rows) {  // (without rows the zeroes of mosaic_run stand)
    ShareTable T{};
    T.slots = (uint64_t)G * G;
    T.sums = swg_alloc<unsigned long long>(ctx, T.slots);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(T.sums, 0, T.slots * sizeof(unsigned long long), st));
    SWG_LAUNCH(ctx, "mosaic_share", mosaic_share_kernel<<<grid_for(ctx, n_rows), TB, 0, st>>>(rows, n_rows, axis ? d.q_id : d.t_id, d.seq_genome, G, T));
    SWG_KERNEL_CHECK(ctx);
    SWG_HIP(ctx, hipMemcpyAsync(req->share, T.sums, T.slots * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SWG_HIP(ctx, hipStreamSynchronize(st));
  }
  return SWG_OK;
}

// the seams' argument checks, then the device work inside an arena frame.  by_length: the weight is the length on the axis
int mosaic_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
               swg_mosaic_request* req, bool by_length, std::vector<swg_mosaic_row>* vec) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: NULL records or request");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: reserved must be 0");
  const uint32_t want = req->want;
  if (want == 0 || want >> 2) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: want names nothing, or a bit beyond the two");
  if (req->axis > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: axis is 0 (query) or 1 (target)");
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: set is SWG_IV_ALL or SWG_IV_KEPT");
  if (!status && req->set == SWG_IV_KEPT) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: the KEPT set needs a status column");
  if ((want & SWG_MOSAIC_SHARE) && !req->share) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: the share bit with a NULL share");
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  SWG_TRY(swg_union_tiles::seg_check_args(ctx, "mosaic", ARG_LIMIT, rec, seq_genome, n_genome, 31));
  if ((want & SWG_MOSAIC_SHARE) && n_genome > MAX_SHARE_GENOMES)
    return swg_set_error(ctx, SWG_ERR_RANGE, "mosaic: a share of more than 4096 genomes (the rows alone have no such limit)");
  const uint32_t* weight = by_length ? nullptr : req->weight ? req->weight : rec->matches;
  if (n) {
    if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end)
      return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: NULL column (q_id, t_id and the four coordinates are read)");
    if (!seq_genome) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: NULL seq_genome");
    if (!by_length && !weight) return swg_set_error(ctx, SWG_ERR_INVALID, "mosaic: NULL weight and NULL matches column");
    SWG_TRY(swg_union_tiles::seg_check_args(ctx, "mosaic", ARG_COUNTS, rec, seq_genome, n_genome, 31));
  }
  // (every refusal of the arguments lies above: none of them touches the caller's outputs)
  if (want & SWG_MOSAIC_ROWS) {
    req->n = req->bases = 0;
    if (vec) vec->clear();
  }
  if (want & SWG_MOSAIC_SHARE) std::memset(req->share, 0, (size_t)n_genome * n_genome * sizeof(uint64_t));
  if (n == 0) return SWG_OK;
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 112 + (size_t)n_seq * 4 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    SegCols d;
    SWG_TRY(swg_union_tiles::seg_stage(ctx, rec, on_device, seq_genome, status, &d));
    const uint32_t* d_weight = weight;
    if (!on_device) {
      swg_stager s(ctx);
      s.add(&d_weight, n);
      SWG_TRY(s.run());
    }
    return mosaic_device(ctx, n, n_seq, n_genome, d, d_weight, req, vec);
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                swg_mosaic_request* req) {
  try {
    return mosaic_run(ctx, rec, on_device, seq_genome, n_genome, status, req, false, nullptr);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

extern "C" int swg_mosaic_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                                  swg_mosaic_request* req) {
  return records_abi(ctx, rec, false, seq_genome, n_genome, status, req);
}

extern "C" int swg_mosaic_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                                         swg_mosaic_request* req) {
  return records_abi(ctx, rec, true, seq_genome, n_genome, status, req);
}

// The mosaic texts of an open PAF: records and genome map from the handle (the last-'#' map of swg_paf_breadth), rows and share
// from ONE device call, the formatting in host/mosaic_text.cpp.  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_mosaic(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t axis, uint32_t set, int by_length, char* out_text[2],
                              uint64_t out_len[2]) {
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_mosaic: NULL argument");
  const bool wanted[2] = {out_text[0] != nullptr, out_text[1] != nullptr};
  out_text[0] = out_text[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_mosaic: neither text is asked for");
  if (axis > 1) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_mosaic: axis is 0 (query) or 1 (target)");
  if (set > 1) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_mosaic: set is SWG_IV_ALL or SWG_IV_KEPT");
  if (set == SWG_IV_KEPT && !status) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_mosaic: the kept set needs a status column");
  const uint64_t n = swg_paf_records(p)->n;
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))  // (before the context is looked at)
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "swg_paf_mosaic: the file has a value >= 2^32, its columns are rebased: the mosaic of 64-bit columns is not supported");
  if (n && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_mosaic: NULL context");
  try {
    std::vector<swg_mosaic_row> rows;
    std::vector<uint64_t> share;
    std::vector<std::string> gname;
    std::vector<uint32_t> col10;  // (rec.matches may point into it: it outlives the text)
    swg_records rec{};
    uint64_t bases = 0;
    if (n) {
      const uint32_t* seq_genome = nullptr;
      SWG_TRY(swg_paf_stats_prepare(p, &rec, &col10, &seq_genome));
      const uint32_t G = rec.n_genome_last;
      swg_mosaic_request req{};
      req.axis = axis, req.set = set;
      if (wanted[0]) req.want |= SWG_MOSAIC_ROWS;
      if (wanted[1]) {
        if (G > MAX_SHARE_GENOMES) return swg_alnstats_error(SWG_ERR_RANGE, "swg_paf_mosaic: the share table takes at most 4096 genomes");
        req.want |= SWG_MOSAIC_ROWS | SWG_MOSAIC_SHARE;  // (the rows bit brings the #total line; no rows are copied without text 0)
        share.assign((size_t)G * G, 0);
        req.share = share.data();
      }
      const int rc = mosaic_run(ctx, &rec, false, seq_genome, G, status, &req, by_length != 0, wanted[0] ? &rows : nullptr);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      bases = req.bases;
      swg_paf_stats_genome_names(p, &gname);
    }
    const std::string text[2] = {wanted[0] ? swg_mosaic_rows_text(p, &rec, rows, axis, by_length != 0) : std::string(),
                                 wanted[1] ? swg_mosaic_share_text(gname, share, bases) : std::string()};
    return texts_hand_over(text, wanted, 2, out_text, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
