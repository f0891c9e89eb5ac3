// The walk over merged intervals (DESIGN.md sections 17, 18, 20 and 21), shared by swg_breadth.hip, swg_intervals.hip and
// swg_sharing.hip (the unit is a sweep segment) and swg_blocks.hip (the unit is a chain).  All sort key = unit << 32 | start with
// the record index as value and then walk the sorted order in tiles of TILE records, ITEMS consecutive ones per thread:
//
//   load_tile / load_ends   a thread's ITEMS keys, values and (second pass) ends, 16-byte loads inside the array
//   gather_tile             first pass: end = end_column[record] written in sorted order, and the tile's maximum of
//                           P = unit << 32 | end -- over all records and, with KEPT, over those whose value carries KEPT_FLAG
//                           (with SKIP_EMPTY: over the records of non-zero length only -- intervals and sharing, which have to say
//                           where an interval begins, need a maximum that no empty record has raised; with TWO_AXES: the
//                           value's AXIS_FLAG picks the end column -- sharing sorts both axes of a record together).
//                           Units ascend along the sorted order, so the maximum of P over any prefix belongs to the LAST unit of
//                           the prefix: a plain running maximum of P is the segmented running maximum of the ends.  The carry
//                           across work-groups is swg_inclusive_max_scan_u64 over these maxima; no work-group waits for another.
//   running_max_before      second pass: the maximum of P over everything in front of a thread -- wavefront scan, the wavefronts
//                           before through LDS, the scanned maxima of the tiles before.  The one place where a tile edge is
//                           crossed: breadth_union, blocks_union and heads_tile all go through it.
//   heads_tile              second and third pass of intervals and sharing: the heads of the merged intervals per set (ALL,
//                           KEPT), counted or, with their ranks, handed to the caller's emitter -- rows in swg_intervals.hip,
//                           begin and end events in swg_sharing.hip.
//   block_sum, bases_sum    a work-group's sum in thread 0; sum(end - start) over a row list
//
// The segment as a unit (breadth, intervals, sharing): SegMap, segmap_alloc (the product or the hashed set), segment_keys (the
// body of a keys kernel), segment_of (segment -> sequence and genome of the other side), and the host front end those three
// share: SegCols, seg_check_args, seg_stage.  rows_hand_over gives a device row list to the caller (intervals, sharing).
// Blocks use the tile, the gather and the running maximum only.
//
// A kernel keeps its own __global__ entry (the profile's launch labels are kernel names); what a pass does with the running
// maximum -- breadth's pair table, blocks' chain rows, the emitters -- stays in the kernel's file.
#pragma once
#include <cstdlib>
#include <vector>

#include "swg_pair_table.h"

namespace swg_union_tiles {

using swg_pair_table::TB;
using swg_pair_table::WAVES;
constexpr int ITEMS = 4;                   // consecutive sorted records per thread
constexpr int TILE = TB * ITEMS;           // ... per work-group
constexpr uint32_t KEPT_FLAG = 0x80000000u;  // bit 31 of a value (n < 2^31 leaves it free)
constexpr uint32_t INDEX_MASK = 0x7fffffffu;
constexpr uint32_t AXIS_FLAG = 0x40000000u;  // TWO_AXES: bit 30 of a value, the entry is the record's target side (n < 2^30)

struct SegMap {  // segment id -> sequence of the axis * G + genome of the other side
  unsigned long long* set_keys;  // hashed: the set (segment = slot); nullptr = the product itself
  uint32_t set_mask;
  uint32_t G;
  uint32_t sentinel;
};

inline bool segmap_forced() {  // test knob: the hashed segment set (and breadth's hashed pair table) at any size
  const char* knob = std::getenv("SWG_BREADTH_HASH");
  return knob && knob[0] == '1';
}

// segments: the product while it (and the sentinel one past it) fits 32 bits, else slots of a set with room for twice the
// segments that can occur -- never more than 2^31 slots, so that slot and sentinel fit too (n < 2^31: a free slot always comes).
// The set comes from the running arena frame; the caller clears it (0xff) ahead of every axis' keys kernel.
inline void segmap_alloc(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, bool force_hash, SegMap* M) {
  const uint64_t products = (uint64_t)n_seq * G;
  *M = SegMap{};
  M->G = G;
  if (products <= 0xffffffffull && !force_hash) {
    M->sentinel = (uint32_t)products;
  } else {
    const uint64_t want = swg_pair_table::pow2_at_least(2 * (products < n ? products : n));
    const uint64_t set_cap = want < (uint64_t(1) << 31) ? want : uint64_t(1) << 31;
    M->set_keys = swg_alloc<unsigned long long>(ctx, set_cap);
    M->set_mask = (uint32_t)(set_cap - 1);
    M->sentinel = (uint32_t)set_cap;
  }
}

// ---- the host front end of breadth, intervals and sharing ------------------------------------------------------------------
struct SegCols {  // the columns a segment walk reads, on the device
  const uint32_t *q_id, *t_id, *start[2], *end[2], *seq_genome;
  const uint8_t* status;
  const uint32_t* seq_len = nullptr;  // sharing only, optional
};

// The argument checks the three share, `which` of them, always in this order (breadth's; intervals and sharing ask for the
// record limit first and for the others later, as they always did, so an input with two faults names the same one as before).
enum : uint32_t { ARG_COLUMNS = 1u, ARG_COUNTS = 2u, ARG_LIMIT = 4u };
inline int seg_check_args(swg_ctx* ctx, const char* who, uint32_t which, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                          int limit_bits) {
  if ((which & ARG_COLUMNS) && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !seq_genome))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL column (q_id, t_id, the four coordinates and seq_genome are read)", who);
  if ((which & ARG_COUNTS) && (rec->n_seq == 0 || n_genome == 0))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: records without sequences or genomes", who);
  if ((which & ARG_LIMIT) && rec->n >= (uint64_t(1) << limit_bits))
    return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^%d records or more in one call", who, limit_bits);
  if ((which & ARG_COUNTS) && rec->n_seq > (uint32_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: more than 2^31 sequences", who);
  return SWG_OK;
}

// inside an arena frame: the columns where they are (on_device), else the six columns, seq_genome and the status staged there
inline int seg_stage(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, const uint8_t* status, SegCols* d) {
  *d = SegCols{rec->q_id, rec->t_id, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, seq_genome, status};
  if (on_device) return SWG_OK;
  swg_stager s(ctx);
  for (const uint32_t** col : {&d->q_id, &d->t_id, &d->start[0], &d->start[1], &d->end[0], &d->end[1]}) s.add(col, rec->n);
  s.add(&d->seq_genome, rec->n_seq);
  s.add(&d->status, rec->n);
  return s.run();
}

// a list's rows from the device to where the caller wants them: `vec` (internal callers), else `rows` when they fit `capacity`.
// *dst: where they went, nullptr = nowhere
template <class Row>
int rows_hand_over(swg_ctx* ctx, const Row* d_rows, uint64_t n_rows, std::vector<Row>* vec, Row* rows, uint64_t capacity, Row** dst) {
  *dst = nullptr;
  if (vec) {
    vec->resize(n_rows);
    *dst = vec->data();
  } else if (rows && n_rows <= capacity) {
    *dst = rows;
  }
  if (!*dst || !n_rows) return SWG_OK;
  SWG_HIP(ctx, hipMemcpyAsync(*dst, d_rows, n_rows * sizeof(Row), hipMemcpyDeviceToHost, ctx->stream));
  SWG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWG_OK;
}

#ifdef __HIPCC__
// The body of a keys kernel, one thread per record, launched over n in work-groups of TB: key = segment << 32 | start, value =
// record index | KEPT_FLAG.  Records that do not count get the segment `sentinel`; an id out of range sets *bad.
template <int AXIS>
__device__ __forceinline__ void segment_keys(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                             const uint32_t* __restrict__ start, const uint8_t* __restrict__ status,
                                             const uint32_t* __restrict__ seq_genome, uint32_t n_seq, const SegMap& M,
                                             uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, unsigned long long* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = q_id[i], t = t_id[i];
  const uint32_t gq = q < n_seq ? seq_genome[q] : swg_pair_table::NONE32, gt = t < n_seq ? seq_genome[t] : swg_pair_table::NONE32;
  uint64_t key = (uint64_t)M.sentinel << 32;
  if (gq >= M.G || gt >= M.G) {
    atomicOr(bad, 1ull);
  } else if (gq != gt) {
    const unsigned long long product = (unsigned long long)(AXIS ? t : q) * M.G + (AXIS ? gq : gt);
    const uint32_t seg = M.set_keys ? swg_pair_table::table_slot(M.set_keys, M.set_mask, product) : (uint32_t)product;
    key = ((uint64_t)seg << 32) | start[i];
  }
  keys[i] = key;
  vals[i] = (uint32_t)i | (status && status[i] != 0 ? KEPT_FLAG : 0u);
}

__device__ __forceinline__ void segment_of(const SegMap& M, uint32_t seg, uint32_t* seq, uint32_t* other) {
  if (M.set_keys) {
    const unsigned long long product = M.set_keys[seg];
    *seq = (uint32_t)(product / M.G), *other = (uint32_t)(product % M.G);
  } else {
    *seq = seg / M.G, *other = seg % M.G;
  }
}

__device__ __forceinline__ void load_tile(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t n, uint64_t p0,
                                          uint64_t (&k)[ITEMS], uint32_t (&v)[ITEMS]) {
  if (p0 + ITEMS <= n) {  // (arena blocks are 16-byte aligned and p0 is a multiple of 4)
    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(keys + p0), b = *reinterpret_cast<const ulonglong2*>(keys + p0 + 2);
    const uint4 w = *reinterpret_cast<const uint4*>(vals + p0);
    k[0] = a.x, k[1] = a.y, k[2] = b.x, k[3] = b.y;
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      k[j] = p0 + j < n ? keys[p0 + j] : ~0ull;
      v[j] = p0 + j < n ? vals[p0 + j] : 0u;
    }
  }
}

__device__ __forceinline__ void load_ends(const uint32_t* __restrict__ ends, uint64_t n, uint64_t p0, uint32_t (&e)[ITEMS]) {
  if (p0 + ITEMS <= n) {
    const uint4 w = *reinterpret_cast<const uint4*>(ends + p0);
    e[0] = w.x, e[1] = w.y, e[2] = w.z, e[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) e[j] = p0 + j < n ? ends[p0 + j] : 0u;
  }
}

__device__ __forceinline__ unsigned long long max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// The body of a gather kernel, launched over the tiles in work-groups of TB.  tile_max: [ntiles] maxima over all records and,
// with KEPT, [ntiles] more over the flagged ones.  `sentinel`: the unit of the records that do not count (sorted to the end).
// `heads` (optional): the number of units that occur is added to it.  TWO_AXES: end_col is the query end column, end_col_t the
// target one.
template <bool KEPT, bool SKIP_EMPTY = false, bool TWO_AXES = false>
__device__ __forceinline__ void gather_tile(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                            const uint32_t* __restrict__ end_col, uint32_t sentinel, uint32_t* __restrict__ ends,
                                            unsigned long long* __restrict__ tile_max, uint64_t ntiles, unsigned long long* __restrict__ heads_out,
                                            const uint32_t* __restrict__ end_col_t = nullptr) {
  __shared__ unsigned long long l_max[2][WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint64_t k[ITEMS];
  uint32_t v[ITEMS], e[ITEMS];
  load_tile(keys, vals, n, p0, k, v);
  uint32_t before = p0 > 0 && p0 <= n ? (uint32_t)(keys[p0 - 1] >> 32) : sentinel;  // (the sentinel is never a head's unit)
  unsigned long long m_all = 0, m_kept = 0;
  uint32_t heads = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const uint32_t seg = (uint32_t)(k[j] >> 32);
    const bool counted = p0 + j < n && seg != sentinel;
    if (TWO_AXES)
      e[j] = counted ? ((v[j] & AXIS_FLAG) ? end_col_t : end_col)[v[j] & INDEX_MASK & ~AXIS_FLAG] : 0u;
    else
      e[j] = counted ? end_col[v[j] & INDEX_MASK] : 0u;  // (values are the indices the keys kernel wrote: < n)
    if (counted) {
      const unsigned long long P = ((unsigned long long)seg << 32) | e[j];
      if (!SKIP_EMPTY || e[j] > (uint32_t)k[j]) {
        m_all = max64(m_all, P);
        if (KEPT && (v[j] & KEPT_FLAG)) m_kept = max64(m_kept, P);
      }
      heads += seg != before || p0 + j == 0;
    }
    before = seg;
  }
  if (p0 + ITEMS <= n) {
    *reinterpret_cast<uint4*>(ends + p0) = make_uint4(e[0], e[1], e[2], e[3]);
  } else {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j)
      if (p0 + j < n) ends[p0 + j] = e[j];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    m_all = max64(m_all, __shfl_xor(m_all, d));
    if (KEPT) m_kept = max64(m_kept, __shfl_xor(m_kept, d));
  }
  if (heads_out) {
    const unsigned long long h = swg_pair_table::wave_sum(heads);
    if (lane == 0 && h) atomicAdd(heads_out, h);
  }
  if (lane == 0) l_max[0][wave] = m_all, l_max[1][wave] = m_kept;
  __syncthreads();
  if (threadIdx.x < (KEPT ? 2 : 1)) {
    unsigned long long m = 0;
    for (int w = 0; w < WAVES; ++w) m = max64(m, l_max[threadIdx.x][w]);
    tile_max[threadIdx.x * ntiles + blockIdx.x] = m;
  }
}
// The maximum of P over everything in front of this thread, per set: `mine` is the maximum over the thread's own records,
// l_wave the work-group's scratch, carry the scanned tile maxima ([ntiles] per set).  `scanned`: bit s = the scan of set s was
// run; the carry-in of a set is read only then (what the gather left of the other set is no carry).  Holds the one barrier of
// the prologue: every thread of the work-group calls it, and what was written to LDS before it is visible after it.
template <int SETS>
__device__ __forceinline__ void running_max_before(const unsigned long long (&mine)[SETS], unsigned long long (&l_wave)[SETS][WAVES],
                                                   const unsigned long long* __restrict__ carry, uint64_t ntiles, uint32_t scanned,
                                                   unsigned long long (&r)[SETS]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long inc[SETS];
#pragma unroll
  for (int s = 0; s < SETS; ++s) inc[s] = mine[s];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    unsigned long long o[SETS];
#pragma unroll
    for (int s = 0; s < SETS; ++s) o[s] = __shfl_up(inc[s], d);
#pragma unroll
    for (int s = 0; s < SETS; ++s)
      if (lane >= d) inc[s] = max64(inc[s], o[s]);
  }
  if (lane == 63) {
#pragma unroll
    for (int s = 0; s < SETS; ++s) l_wave[s][wave] = inc[s];
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    r[s] = __shfl_up(inc[s], 1);
    if (lane == 0) r[s] = 0;
  }
  for (int w = 0; w < wave; ++w) {
#pragma unroll
    for (int s = 0; s < SETS; ++s) r[s] = max64(r[s], l_wave[s][w]);
  }
  if (blockIdx.x > 0) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
      if (scanned >> s & 1u) r[s] = max64(r[s], carry[s * ntiles + blockIdx.x - 1]);
  }
}

// One tile of the sorted order: the heads of the sets in `sets` (bit 0 ALL, bit 1 KEPT; their tile maxima are scanned in
// `carry`).  A counted record of non-zero length is a head of its set when nothing of the set came before, or the maximum
// before it belongs to an earlier segment, or start > that maximum's end (strictly: touching intervals join).  WRITE = false:
// the number of heads per set into tile_cnt[s * ntiles + tile]; the emitter is not used.  WRITE = true: tile_cnt holds the
// exclusive scan of those numbers, and the emitter (by value, statically dispatched) gets
//   out.total[s]                  the heads of set s over all tiles
//   out.head(s, at, key, prev)    the head of rank at < total[s]: its key, and the running maximum in front of it -- segment
//                                 and end of the interval of rank at - 1, which it closes (the maximum over a prefix belongs to
//                                 the last segment the set touched); 0 for at == 0
//   out.last(s, max)              once per set with total[s] > 0: the last interval closes at the maximum over everything
template <bool WRITE, class Emit>
__device__ __forceinline__ void heads_tile(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                           const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry, uint64_t ntiles,
                                           uint32_t sentinel, uint32_t sets, uint32_t* __restrict__ tile_cnt, const Emit& out) {
  __shared__ unsigned long long l_wave[2][WAVES];
  __shared__ uint32_t l_cnt[2][WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint64_t k[ITEMS];
  uint32_t v[ITEMS], e[ITEMS];
  load_tile(keys, vals, n, p0, k, v);
  load_ends(ends, n, p0, e);
  bool live[ITEMS];  // counted and of non-zero length
  unsigned long long t_max[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    live[j] = p0 + j < n && (uint32_t)(k[j] >> 32) != sentinel && e[j] > (uint32_t)k[j];
    if (live[j]) {
      const unsigned long long P = (k[j] & 0xffffffff00000000ull) | e[j];
      t_max[0] = max64(t_max[0], P);
      if (v[j] & KEPT_FLAG) t_max[1] = max64(t_max[1], P);
    }
  }
  unsigned long long r[2];
  running_max_before<2>(t_max, l_wave, carry, ntiles, sets, r);
  // heads.  A maximum of 0 is "nothing of the set before": a live record has end >= 1, so its P is never 0.
  uint32_t cnt[2] = {0, 0}, is_head[2] = {0, 0};
  unsigned long long prev[2][ITEMS];  // the running maximum in front of a head
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    prev[0][j] = prev[1][j] = 0;
    if (!live[j]) continue;
    const uint32_t seg = (uint32_t)(k[j] >> 32), start = (uint32_t)k[j];
    const unsigned long long P = (k[j] & 0xffffffff00000000ull) | e[j];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (!(sets >> s & 1u) || (s == 1 && !(v[j] & KEPT_FLAG))) continue;
      if (r[s] == 0 || (uint32_t)(r[s] >> 32) != seg || start > (uint32_t)r[s]) {
        ++cnt[s];
        is_head[s] |= 1u << j;
        prev[s][j] = r[s];
      }
      r[s] = max64(r[s], P);
    }
  }
  if (!WRITE) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint32_t c = (uint32_t)swg_pair_table::wave_sum(cnt[s]);
      if (lane == 0) l_cnt[s][wave] = c;
    }
    __syncthreads();
    if (threadIdx.x < 2 && (sets >> threadIdx.x & 1u)) {
      uint32_t c = 0;
      for (int w = 0; w < WAVES; ++w) c += l_cnt[threadIdx.x][w];
      tile_cnt[threadIdx.x * ntiles + blockIdx.x] = c;
    }
    return;
  }
  // ranks: heads of the threads before this one, of the tiles before this one
  uint32_t rank[2] = {cnt[0], cnt[1]};
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t a = __shfl_up(rank[0], d), b = __shfl_up(rank[1], d);
    if (lane >= d) rank[0] += a, rank[1] += b;
  }
  if (lane == 63) l_cnt[0][wave] = rank[0], l_cnt[1][wave] = rank[1];
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (!(sets >> s & 1u)) continue;
    uint32_t at = rank[s] - cnt[s] + tile_cnt[s * ntiles + blockIdx.x];
    for (int w = 0; w < wave; ++w) at += l_cnt[s][w];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      if (!(is_head[s] >> j & 1u)) continue;
      if (at < out.total[s]) out.head(s, at, k[j], prev[s][j]);  // (always: the count pass counted these heads)
      ++at;
    }
    if (blockIdx.x == ntiles - 1 && threadIdx.x == 0 && out.total[s] > 0) out.last(s, carry[s * ntiles + ntiles - 1]);
  }
}

// v summed over the work-group (l_sum: its scratch): thread 0 returns the total, the other threads 0
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long (&l_sum)[WAVES]) {
  v = swg_pair_table::wave_sum(v);
  if ((threadIdx.x & 63) == 0) l_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < WAVES; ++w) t += l_sum[w];
  return t;
}

// The body of a bases kernel (grid-stride over the rows): sum(end - start) added to *sum, one atomic per work-group
template <class Row>
__device__ __forceinline__ void bases_sum(const Row* __restrict__ rows, uint64_t n_rows, unsigned long long* __restrict__ sum) {
  __shared__ unsigned long long l_sum[WAVES];
  unsigned long long s = 0;
  for (uint64_t x = (uint64_t)blockIdx.x * TB + threadIdx.x; x < n_rows; x += (uint64_t)gridDim.x * TB) s += rows[x].end - rows[x].start;
  const unsigned long long t = block_sum(s, l_sum);
  if (t) atomicAdd(sum, t);
}
#endif

}  // namespace swg_union_tiles
