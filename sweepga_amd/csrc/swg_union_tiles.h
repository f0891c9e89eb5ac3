// Tiles of the merged-interval passes (DESIGN.md sections 17 and 18), shared by swg_breadth.hip (the unit is a sweep segment)
// and swg_blocks.hip (the unit is a chain).  Both sort key = unit << 32 | start with the record index as value and then walk
// the sorted order in tiles of TILE records, ITEMS consecutive ones per thread:
//
//   load_tile / load_ends   a thread's ITEMS keys, values and (second pass) ends, 16-byte loads inside the array
//   gather_tile             first pass: end = end_column[record] written in sorted order, and the tile's maximum of
//                           P = unit << 32 | end -- over all records and, with KEPT, over those whose value carries KEPT_FLAG.
//                           Units ascend along the sorted order, so the maximum of P over any prefix belongs to the LAST unit of
//                           the prefix: a plain running maximum of P is the segmented running maximum of the ends.  The carry
//                           across work-groups is swg_inclusive_max_scan_u64 over these maxima; no work-group waits for another.
//
// A kernel keeps its own __global__ entry (the profile's launch labels are kernel names) and its own second pass.
#pragma once
#include "swg_pair_table.h"

namespace swg_union_tiles {

using swg_pair_table::TB;
using swg_pair_table::WAVES;
constexpr int ITEMS = 4;                   // consecutive sorted records per thread
constexpr int TILE = TB * ITEMS;           // ... per work-group
constexpr uint32_t KEPT_FLAG = 0x80000000u;  // bit 31 of a value (n < 2^31 leaves it free)
constexpr uint32_t INDEX_MASK = 0x7fffffffu;

#ifdef __HIPCC__
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
// `heads` (optional): the number of units that occur is added to it.
template <bool KEPT>
__device__ __forceinline__ void gather_tile(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                            const uint32_t* __restrict__ end_col, uint32_t sentinel, uint32_t* __restrict__ ends,
                                            unsigned long long* __restrict__ tile_max, uint64_t ntiles, unsigned long long* __restrict__ heads_out) {
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
    e[j] = counted ? end_col[v[j] & INDEX_MASK] : 0u;  // (values are the indices the keys kernel wrote: < n)
    if (counted) {
      const unsigned long long P = ((unsigned long long)seg << 32) | e[j];
      m_all = max64(m_all, P);
      if (KEPT && (v[j] & KEPT_FLAG)) m_kept = max64(m_kept, P);
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
