// Tiles of the merged-interval passes (DESIGN.md sections 17 and 18), shared by swg_breadth.hip (the unit is a sweep segment)
// and swg_blocks.hip (the unit is a chain).  Both sort key = unit << 32 | start with the record index as value and then walk
// the sorted order in tiles of TILE records, ITEMS consecutive ones per thread:
//
//   load_tile / load_ends   a thread's ITEMS keys, values and (second pass) ends, 16-byte loads inside the array
//   gather_tile             first pass: end = end_column[record] written in sorted order, and the tile's maximum of
//                           P = unit << 32 | end -- over all records and, with KEPT, over those whose value carries KEPT_FLAG
//                           (with SKIP_EMPTY: over the records of non-zero length only -- swg_intervals.hip, which has to say
//                           where an interval begins, needs a maximum that no empty record has raised; with TWO_AXES: the
//                           value's AXIS_FLAG picks the end column -- swg_sharing.hip sorts both axes of a record together).
//                           Units ascend along the sorted order, so the maximum of P over any prefix belongs to the LAST unit of
//                           the prefix: a plain running maximum of P is the segmented running maximum of the ends.  The carry
//                           across work-groups is swg_inclusive_max_scan_u64 over these maxima; no work-group waits for another.
//
// The segment as a unit is shared by swg_breadth.hip and swg_intervals.hip: SegMap, segmap_alloc (the product or the hashed set)
// and segment_keys (the body of a keys kernel).
//
// A kernel keeps its own __global__ entry (the profile's launch labels are kernel names) and its own second pass.
#pragma once
#include <cstdlib>

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
#endif

}  // namespace swg_union_tiles
