// Intervals: WHERE the coverage of section 17 lies.  Per unit -- breadth's sweep segment, one sequence
// against one genome of the other side, inter-genome records only -- and per axis three lists of maximal half-open intervals:
//
//   ALL   the union of [start, end) over the counted records          KEPT  the same over the records with status != 0
//   LOST  ALL minus KEPT: covered before the filter, by nothing after it
//
// each ordered by (sequence, genome of the other side, start).  Keys, sort, the tile walk and the head rule are shared
// (swg_union_tiles.h: segment_keys, gather_tile, running_max_before, heads_tile); this file holds what a head writes (RowsOut):
//
//   intervals_keys        key = segment << 32 | start, value = record index | KEPT_FLAG (segment_keys)
//   (sort)                swg_radix_sort_pairs
//   intervals_gather      end = end_column[record] in sorted order, and the tile maxima of P = segment << 32 | end for ALL and
//                         KEPT -- over the records of NON-ZERO length only (gather_tile<true, true>).  Breadth may let an empty
//                         record raise the maximum, because it only sums; here an empty record at p would make an interval that
//                         really begins at p after a gap look like a continuation and glue it to the interval before the gap.
//   (scan)                swg_inclusive_max_scan_u64 over the tile maxima: the carry, however far it reaches
//   intervals_count       the tile again (heads_tile<false>).  Running maximum before each record (wavefront shuffles, wavefronts through LDS,
//                         carry-in from the scan).  A counted record of non-zero length is a HEAD of its set when nothing of the
//                         set came before, or the maximum before it belongs to an earlier segment, or start > that maximum's
//                         end (strictly: touching intervals join).  Heads per tile and set.
//   (scan)                swg_exclusive_scan_u32 over the tile counts; the totals are the lists' n.  One read-back sizes the rows.
//   intervals_write       the tile a third time (heads_tile<true> with RowsOut).  The head of rank r writes
//                         row[r].{seq, other_genome, start} and, if r > 0, row[r - 1].end = the low half of the running maximum before it: the maximum of P over a prefix
//                         belongs to the last segment the set touched, so it IS the previous interval's end, also when that
//                         interval lies in another segment.  The last row's end is the low half of the last tile's scanned
//                         maximum.  No look-ahead, no atomics, no neighbour's state.  Launched only for an axis and sets whose
//                         rows are wanted (LOST wants both).
//   intervals_lost_flags  over the two row lists, by their keys segment << 32 | start: a thread per ALL row A finds the first
//                         KEPT row with key >= its own (binary search): the leading piece is [A.start, K.start) if that K lies
//                         in A, all of A if none does, nothing if K starts at A.start.  A thread per KEPT row K finds the A
//                         that holds it: the trailing piece is [K.end, next K.start if that lies in the same A, else A.end).
//   (scans)               two swg_exclusive_scan_u32 over the flags; a second read-back sizes the LOST rows.
//   intervals_lost_write  rank of a leading piece = leading pieces of the A rows before it + trailing pieces of the K rows
//                         before its first K; of a trailing piece = leading pieces up to its A + trailing pieces before it.
//                         Scattered by rank: exact order, no atomics.
//   intervals_bases       sum(end - start) over a row list: work-group reduction, one atomic per work-group (bases_sum).
//
// No work-group waits for another inside a launch (no look-back, no flag): every carry goes through the library's scans
// between launches.  With the hashed segment set (beyond 2^32 products; SWG_BREADTH_HASH=1) segments are hash slots and the
// device order is by slot: the host then orders whole segment runs by (sequence, genome) with a stable sort -- the rows of a
// run are in start order already.  Integer atomics only; no floating point.
#include <algorithm>
#include <new>
#include <string>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;
using namespace swg_union_tiles;
// device scalars: an id out of range, then per axis the heads of ALL and KEPT, the leading and trailing pieces, the bases of the
// three lists
enum { D_BAD = 0, D_AXIS = 1, A_HEADS = 0, A_LEAD = 2, A_TRAIL = 3, A_BASES = 4, A_COUNT = 8, D_TOTAL = D_AXIS + 2 * A_COUNT };
constexpr uint32_t SET_ALL = 1u, SET_KEPT = 2u;

template <int AXIS>
__global__ __launch_bounds__(TB) void intervals_keys_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                            const uint32_t* __restrict__ start, const uint8_t* __restrict__ status,
                                                            const uint32_t* __restrict__ seq_genome, uint32_t n_seq, SegMap M,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                            unsigned long long* __restrict__ scalars) {
  segment_keys<AXIS>(n, q_id, t_id, start, status, seq_genome, n_seq, M, keys, vals, &scalars[D_BAD]);
}

__global__ __launch_bounds__(TB) void intervals_gather_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                              const uint32_t* __restrict__ end_col, uint32_t sentinel,
                                                              uint32_t* __restrict__ ends, unsigned long long* __restrict__ tile_max, uint64_t ntiles) {
  gather_tile<true, true>(n, keys, vals, end_col, sentinel, ends, tile_max, ntiles, nullptr);
}

struct RowsOut {           // the write pass' emitter (heads_tile, swg_union_tiles.h): the rows per set (ALL, KEPT)
  SegMap M;
  swg_interval* rows[2];   // [total[s]]
  uint64_t* keys[2];       // [total[s]] segment << 32 | start of every row, or nullptr (only the LOST stage reads them)
  uint32_t total[2];
  // the head of rank `at` begins row at and closes row at - 1 at the low half of the maximum in front of it
  __device__ __forceinline__ void head(int s, uint32_t at, uint64_t key, unsigned long long prev) const {
    swg_interval* row = rows[s] + at;
    segment_of(M, (uint32_t)(key >> 32), &row->seq, &row->other_genome);
    row->start = (uint32_t)key;
    if (at > 0) row[-1].end = (uint32_t)prev;
    if (keys[s]) keys[s][at] = key;
  }
  __device__ __forceinline__ void last(int s, unsigned long long max_p) const { rows[s][total[s] - 1].end = (uint32_t)max_p; }
};

__global__ __launch_bounds__(TB) void intervals_count_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                             const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry,
                                                             uint64_t ntiles, SegMap M, uint32_t sets, uint32_t* __restrict__ tile_cnt) {
  heads_tile<false>(n, keys, vals, ends, carry, ntiles, M.sentinel, sets, tile_cnt, RowsOut{});
}

__global__ __launch_bounds__(TB) void intervals_write_kernel(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                             const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry,
                                                             uint64_t ntiles, uint32_t sets, uint32_t* __restrict__ tile_off, RowsOut out) {
  heads_tile<true>(n, keys, vals, ends, carry, ntiles, out.M.sentinel, sets, tile_off, out);
}

// ---- LOST = ALL minus KEPT over the two row lists ---------------------------------------------------------------------------
struct LostArgs {
  const swg_interval *a_rows, *k_rows;
  const uint64_t *a_keys, *k_keys;  // segment << 32 | start, ascending
  uint32_t n_a, n_k;
  uint32_t* flag;  // [n_a + n_k]: A row has a leading piece; K row has a trailing piece (then: their exclusive scans)
  uint32_t* link;  // [n_a + n_k]: A row -> its first K row with key >= its own; K row -> the A row that holds it
};

__device__ __forceinline__ uint32_t first_at_least(const uint64_t* __restrict__ keys, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the trailing piece of K row j inside A row i: [K.end, next K.start if that K lies in the same A, else A.end)
__device__ __forceinline__ void trailing_piece(const LostArgs& L, uint32_t i, uint32_t j, uint32_t* from, uint32_t* to) {
  *from = L.k_rows[j].end;
  *to = L.a_rows[i].end;
  if (j + 1 < L.n_k && (L.k_keys[j + 1] >> 32) == (L.a_keys[i] >> 32) && (uint32_t)L.k_keys[j + 1] < *to) *to = (uint32_t)L.k_keys[j + 1];
}

__global__ __launch_bounds__(TB) void intervals_lost_flags_kernel(LostArgs L) {
  const uint64_t x = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (x < L.n_a) {
    const uint32_t i = (uint32_t)x;
    const uint64_t key = L.a_keys[i];
    const uint32_t j = first_at_least(L.k_keys, L.n_k, key);
    // (K rows lie inside A rows: a K of this segment at or after A.start and before A.end lies in this A)
    const bool inside = j < L.n_k && (L.k_keys[j] >> 32) == (key >> 32) && (uint32_t)L.k_keys[j] < L.a_rows[i].end;
    L.link[i] = j;
    L.flag[i] = !inside || (uint32_t)L.k_keys[j] > (uint32_t)key;
  } else if (x < (uint64_t)L.n_a + L.n_k) {
    const uint32_t j = (uint32_t)(x - L.n_a);
    const uint32_t i = first_at_least(L.a_keys, L.n_a, L.k_keys[j] + 1) - 1;  // the last A with key <= K's: every K has one
    uint32_t from = 0, to = 0;
    if (i < L.n_a) trailing_piece(L, i, j, &from, &to);  // (always: every KEPT interval lies inside an ALL interval)
    L.link[x] = i < L.n_a ? i : 0u;
    L.flag[x] = to > from;
  }
}

// L.flag now holds the exclusive scans of its two halves (leading pieces of the A rows, trailing pieces of the K rows): a row
// has a piece when the next entry -- the total behind the last one -- is larger than its own
__global__ __launch_bounds__(TB) void intervals_lost_write_kernel(LostArgs L, uint32_t n_lead, uint32_t n_trail, swg_interval* __restrict__ rows) {
  const uint64_t x = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const uint32_t* lead = L.flag;
  const uint32_t* trail = L.flag + L.n_a;
  const uint32_t n_rows = n_lead + n_trail;
  if (x < L.n_a) {
    const uint32_t i = (uint32_t)x, j = L.link[i];
    const uint32_t mine = lead[i], next = i + 1 < L.n_a ? lead[i + 1] : n_lead;
    if (next == mine) return;
    const swg_interval a = L.a_rows[i];
    const bool inside = j < L.n_k && (L.k_keys[j] >> 32) == (L.a_keys[i] >> 32) && (uint32_t)L.k_keys[j] < a.end;
    const uint32_t at = mine + (j < L.n_k ? trail[j] : n_trail);
    if (at < n_rows) rows[at] = swg_interval{a.seq, a.other_genome, a.start, inside ? (uint32_t)L.k_keys[j] : a.end};
  } else if (x < (uint64_t)L.n_a + L.n_k) {
    const uint32_t j = (uint32_t)(x - L.n_a), i = L.link[x];
    const uint32_t mine = trail[j], next = j + 1 < L.n_k ? trail[j + 1] : n_trail;
    if (next == mine) return;
    uint32_t from, to;
    trailing_piece(L, i, j, &from, &to);
    const uint32_t at = (i + 1 < L.n_a ? lead[i + 1] : n_lead) + mine;
    if (at < n_rows) rows[at] = swg_interval{L.a_rows[i].seq, L.a_rows[i].other_genome, from, to};
  }
}

__global__ __launch_bounds__(TB) void intervals_bases_kernel(const swg_interval* __restrict__ rows, uint64_t n_rows, unsigned long long* __restrict__ sum) {
  bases_sum(rows, n_rows, sum);
}

// a list's n, bases and rows to the caller (rows_hand_over); the hashed set's rows into their order on the way
int hand_over(swg_ctx* ctx, const swg_interval* d_rows, uint64_t n_rows, uint64_t bases, bool hashed, swg_interval_list* list,
              std::vector<swg_interval>* vec) {
  list->n = n_rows;
  list->bases = bases;
  swg_interval* dst;
  SWG_TRY(rows_hand_over(ctx, d_rows, n_rows, vec, list->rows, list->capacity, &dst));
  if (dst && hashed)  // the device order is by hash slot: whole segment runs into (sequence, genome) order, their rows stay in start order
    std::stable_sort(dst, dst + n_rows, [](const swg_interval& a, const swg_interval& b) {
      return a.seq != b.seq ? a.seq < b.seq : a.other_genome < b.other_genome;
    });
  return SWG_OK;
}

// inside an arena frame.  vecs: nullptr, or [3][2] vectors that receive the rows instead of req's arrays
int intervals_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const SegCols& d, swg_interval_request* req,
                     std::vector<swg_interval> (*vecs)[2]) {
  hipStream_t st = ctx->stream;
  const bool force_hash = segmap_forced();
  const uint64_t ntiles = (n + TILE - 1) / TILE;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  uint64_t* keys = swg_alloc<uint64_t>(ctx, n);
  uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n);
  uint32_t* vals = swg_alloc<uint32_t>(ctx, n);
  uint32_t* vals_alt = swg_alloc<uint32_t>(ctx, n);
  uint32_t* ends = swg_alloc<uint32_t>(ctx, n);
  unsigned long long* tile_max = swg_alloc<unsigned long long>(ctx, 2 * ntiles);
  uint32_t* tile_cnt = swg_alloc<uint32_t>(ctx, 2 * ntiles);
  SegMap M;
  segmap_alloc(ctx, n, n_seq, G, force_hash, &M);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  const int end_bit = 32 + swg_bits_for(M.sentinel);
  const unsigned grid_n = (unsigned)((n + TB - 1) / TB), grid_t = (unsigned)ntiles;
  for (int axis = 0; axis < 2; ++axis) {
    const bool want[3] = {(req->want >> (2 * SWG_IV_ALL + axis) & 1u) != 0, (req->want >> (2 * SWG_IV_KEPT + axis) & 1u) != 0,
                          (req->want >> (2 * SWG_IV_LOST + axis) & 1u) != 0};
    if (!want[0] && !want[1] && !want[2]) continue;
    const uint32_t sets = (want[0] || want[2] ? SET_ALL : 0u) | (want[1] || want[2] ? SET_KEPT : 0u);
    unsigned long long* ax = scalars + D_AXIS + axis * A_COUNT;
    const swg_arena_mark mark = swg_arena_save(ctx);  // (the rows of this axis go back to the arena behind it)
    if (M.set_keys) SWG_HIP(ctx, hipMemsetAsync(M.set_keys, 0xff, ((size_t)M.set_mask + 1) * sizeof(unsigned long long), st));
    if (axis == 0)
      SWG_LAUNCH(ctx, "intervals_keys", intervals_keys_kernel<0><<<grid_n, TB, 0, st>>>(n, d.q_id, d.t_id, d.start[0], d.status, d.seq_genome,
                                                                                         n_seq, M, keys, vals, scalars));
    else
      SWG_LAUNCH(ctx, "intervals_keys", intervals_keys_kernel<1><<<grid_n, TB, 0, st>>>(n, d.q_id, d.t_id, d.start[1], d.status, d.seq_genome,
                                                                                         n_seq, M, keys, vals, scalars));
    SWG_KERNEL_CHECK(ctx);
    {
      swg_prof_scope sort_scope(ctx, axis == 0 ? "intervals_sort_q" : "intervals_sort_t");
      SWG_TRY(swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, n, 0, end_bit));
    }
    SWG_LAUNCH(ctx, "intervals_gather", intervals_gather_kernel<<<grid_t, TB, 0, st>>>(n, keys, vals, d.end[axis], M.sentinel, ends, tile_max, ntiles));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max), reinterpret_cast<uint64_t*>(tile_max), ntiles));
    if (sets & SET_KEPT)
      SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max + ntiles), reinterpret_cast<uint64_t*>(tile_max + ntiles), ntiles));
    SWG_LAUNCH(ctx, "intervals_count", intervals_count_kernel<<<grid_t, TB, 0, st>>>(n, keys, vals, ends, tile_max, ntiles, M, sets, tile_cnt));
    SWG_KERNEL_CHECK(ctx);
    for (int s = 0; s < 2; ++s)
      if (sets >> s & 1u)
        SWG_TRY(swg_exclusive_scan_u32(ctx, tile_cnt + s * ntiles, tile_cnt + s * ntiles, ntiles, reinterpret_cast<uint64_t*>(ax + A_HEADS + s)));
    uint64_t h[D_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
    if (h[D_BAD]) return swg_set_error(ctx, SWG_ERR_INVALID, "intervals: a sequence id >= n_seq or a genome id >= n_genome");
    const uint64_t* hx = h + D_AXIS + axis * A_COUNT;
    RowsOut out{};
    out.M = M;
    for (int s = 0; s < 2; ++s) {
      if (!(sets >> s & 1u)) continue;
      out.total[s] = (uint32_t)hx[A_HEADS + s];  // (<= n < 2^31)
      out.rows[s] = swg_alloc<swg_interval>(ctx, out.total[s] ? out.total[s] : 1);
      if (want[2]) out.keys[s] = swg_alloc<uint64_t>(ctx, out.total[s] ? out.total[s] : 1);
    }
    LostArgs L{};
    if (want[2]) {
      L.flag = swg_alloc<uint32_t>(ctx, (uint64_t)out.total[0] + out.total[1] + 1);
      L.link = swg_alloc<uint32_t>(ctx, (uint64_t)out.total[0] + out.total[1] + 1);
    }
    SWG_CHECK_ARENA(ctx);
    SWG_LAUNCH(ctx, "intervals_write", intervals_write_kernel<<<grid_t, TB, 0, st>>>(n, keys, vals, ends, tile_max, ntiles, sets, tile_cnt, out));
    SWG_KERNEL_CHECK(ctx);
    swg_interval* lost_rows = nullptr;
    uint64_t n_lost = 0;
    if (want[2] && out.total[0]) {
      L.a_rows = out.rows[0], L.k_rows = out.rows[1], L.a_keys = out.keys[0], L.k_keys = out.keys[1];
      L.n_a = out.total[0], L.n_k = out.total[1];
      const unsigned grid_l = (unsigned)(((uint64_t)L.n_a + L.n_k + TB - 1) / TB);
      SWG_LAUNCH(ctx, "intervals_lost_flags", intervals_lost_flags_kernel<<<grid_l, TB, 0, st>>>(L));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_exclusive_scan_u32(ctx, L.flag, L.flag, L.n_a, reinterpret_cast<uint64_t*>(ax + A_LEAD)));
      SWG_TRY(swg_exclusive_scan_u32(ctx, L.flag + L.n_a, L.flag + L.n_a, L.n_k, reinterpret_cast<uint64_t*>(ax + A_TRAIL)));
      uint64_t hl[2];
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(ax + A_LEAD), hl, 2));
      n_lost = hl[0] + hl[1];
      lost_rows = swg_alloc<swg_interval>(ctx, n_lost ? n_lost : 1);
      SWG_CHECK_ARENA(ctx);
      if (n_lost) {
        SWG_LAUNCH(ctx, "intervals_lost_write", intervals_lost_write_kernel<<<grid_l, TB, 0, st>>>(L, (uint32_t)hl[0], (uint32_t)hl[1], lost_rows));
        SWG_KERNEL_CHECK(ctx);
      }
    }
    const swg_interval* d_rows[3] = {out.rows[0], out.rows[1], lost_rows};
    const uint64_t n_rows[3] = {out.total[0], out.total[1], n_lost};
    for (int s = 0; s < 3; ++s)
      if (want[s] && n_rows[s]) {
        SWG_LAUNCH(ctx, "intervals_bases", intervals_bases_kernel<<<grid_for(ctx, n_rows[s]), TB, 0, st>>>(d_rows[s], n_rows[s], ax + A_BASES + s));
        SWG_KERNEL_CHECK(ctx);
      }
    uint64_t hb[3];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(ax + A_BASES), hb, 3));
    for (int s = 0; s < 3; ++s)
      if (want[s]) SWG_TRY(hand_over(ctx, d_rows[s], n_rows[s], hb[s], M.set_keys != nullptr, &req->list[s][axis], vecs ? &vecs[s][axis] : nullptr));
    swg_arena_restore(ctx, mark);
  }
  return SWG_OK;
}

// the seams' argument checks, then the device work inside an arena frame
int intervals_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                  swg_interval_request* req, std::vector<swg_interval> (*vecs)[2]) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "intervals: NULL records or request");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "intervals: reserved must be 0");
  if (req->want == 0 || req->want >> 6) return swg_set_error(ctx, SWG_ERR_INVALID, "intervals: want names no list, or a bit beyond the six");
  if (!status && (req->want >> (2 * SWG_IV_KEPT)) != 0)
    return swg_set_error(ctx, SWG_ERR_INVALID, "intervals: the KEPT and LOST lists need a status column");
  const uint64_t n = rec->n;
  SWG_TRY(seg_check_args(ctx, "intervals", ARG_LIMIT, rec, seq_genome, n_genome, 31));
  for (int s = 0; s < 3; ++s)
    for (int axis = 0; axis < 2; ++axis)
      if (req->want >> (2 * s + axis) & 1u) {
        req->list[s][axis].n = req->list[s][axis].bases = 0;
        if (vecs) vecs[s][axis].clear();
      }
  if (n == 0) return SWG_OK;
  SWG_TRY(seg_check_args(ctx, "intervals", ARG_COLUMNS | ARG_COUNTS, rec, seq_genome, n_genome, 31));
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 64 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    SegCols d;
    SWG_TRY(seg_stage(ctx, rec, on_device, seq_genome, status, &d));
    return intervals_device(ctx, n, rec->n_seq, n_genome, d, req, vecs);
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                swg_interval_request* req) {
  try {
    return intervals_run(ctx, rec, on_device, seq_genome, n_genome, status, req, nullptr);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

extern "C" int swg_intervals_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                     const uint8_t* status, swg_interval_request* req) {
  return records_abi(ctx, rec, false, seq_genome, n_genome, status, req);
}

extern "C" int swg_intervals_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                            const uint8_t* status, swg_interval_request* req) {
  return records_abi(ctx, rec, true, seq_genome, n_genome, status, req);
}

// The interval texts of an open PAF: records and genome map from the handle (the last-'#' map of swg_paf_breadth), the rows of
// all the sets asked for from ONE device call, the names from the handle.  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_interval_texts(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, uint32_t sets, char** out_text, uint64_t* out_len) {
  if (out_text && out_len && sets < 8)
    for (int s = 0; s < 3; ++s)
      if (sets >> s & 1u) out_text[s] = nullptr, out_len[s] = 0;
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_intervals: NULL argument");
  if (sets == 0 || sets >= 8) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_intervals: a set outside ALL (0), KEPT (1), LOST (2)");
  if (!status && (sets >> SWG_IV_KEPT) != 0) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_intervals: the KEPT and LOST lists need a status column");
  const uint64_t n = swg_paf_records(p)->n;
  if (n && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_intervals: NULL context");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "swg_paf_intervals: the file has a value >= 2^32, its columns are rebased: intervals of 64-bit columns are not supported");
  try {
    std::vector<swg_interval> rows[3][2];
    std::vector<std::string> gname;
    if (n) {
      swg_records rec;
      std::vector<uint32_t> col10;
      const uint32_t* seq_genome = nullptr;
      SWG_TRY(swg_paf_stats_prepare(p, &rec, &col10, &seq_genome));
      swg_interval_request req{};
      for (int s = 0; s < 3; ++s)
        if (sets >> s & 1u) req.want |= 3u << (2 * s);
      const int rc = intervals_run(ctx, &rec, false, seq_genome, rec.n_genome_last, status, &req, rows);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      swg_paf_stats_genome_names(p, &gname);
    }
    std::string text[3];
    const bool wanted[3] = {(sets & 1u) != 0, (sets & 2u) != 0, (sets & 4u) != 0};
    for (int s = 0; s < 3; ++s) {
      if (!wanted[s]) continue;
      std::string& o = text[s];
      for (int axis = 0; axis < 2; ++axis)
        for (const swg_interval& r : rows[s][axis]) {
          o += swg_paf_sequence_name(p, r.seq);
          o += '\t';
          append_u64(o, r.start, '\t');
          append_u64(o, r.end, '\t');
          o += gname[r.other_genome];
          o += axis ? "\tt\n" : "\tq\n";
        }
    }
    return texts_hand_over(text, wanted, 3, out_text, out_len);
  } catch (const std::bad_alloc&) {  // (no text has been handed over yet: the outputs are as zeroed above)
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_paf_intervals(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, int set, char** out_text, uint64_t* out_len) {
  if (out_text) *out_text = nullptr;
  if (out_len) *out_len = 0;
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_intervals: NULL argument");
  if (set < 0 || set > 2) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_intervals: a set outside ALL (0), KEPT (1), LOST (2)");
  char* text[3] = {nullptr, nullptr, nullptr};
  uint64_t len[3] = {0, 0, 0};
  SWG_TRY(swg_paf_interval_texts(ctx, p, status, 1u << set, text, len));
  *out_text = text[set];
  *out_len = len[set];
  return SWG_OK;
}
