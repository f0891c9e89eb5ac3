// What the per-genome-pair reductions share (swg_alnstats.hip: alnstats' ordered pairs; swg_sparsify.hip: the tree
// sparsification's unordered pairs): runs of one key along the lanes of a wavefront are summed towards the run's first lane,
// the run heads go through a small LDS table of the work-group, and the table is flushed with one atomic per (work-group, key,
// quantity) into a global table that is dense (slot = key) while G x G is small and open addressing beyond.
#pragma once
#include "swg_internal.h"

namespace swg_pair_table {

constexpr int TB = 256;                    // threads per work-group
constexpr int WAVES = TB / 64;
constexpr int LSLOTS = 256;                // LDS genome-pair slots per work-group
constexpr int LPROBES = 8;                 // ... probed this far, then the run goes to the global table directly
constexpr uint32_t NONE32 = 0xffffffffu;
constexpr unsigned long long EMPTY = ~0ull;
constexpr uint64_t DENSE_LIMIT = uint64_t(1) << 20;  // G * G entries

static inline uint64_t pow2_at_least(uint64_t v) {
  uint64_t c = 1024;
  while (c < v) c <<= 1;
  return c;
}

// the slot hash of every open-addressing table here, device and host (a table built on the host is probed on the device)
__host__ __device__ __forceinline__ uint32_t hash32(unsigned long long key) { return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 32); }

#ifdef __HIPCC__
// slot of `key` in an open-addressing key table of mask + 1 slots (EMPTY = free); inserts when absent.  The table has twice
// the slots of the keys that can occur: a free one always comes.
__device__ __forceinline__ uint32_t table_slot(unsigned long long* keys, uint32_t mask, unsigned long long key) {
  uint32_t h = hash32(key) & mask;
  for (;;) {
    unsigned long long k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == EMPTY) {
      k = atomicCAS(&keys[h], EMPTY, key);
      if (k == EMPTY) k = key;
    }
    if (k == key) return h;
    h = (h + 1) & mask;
  }
}

// slot of `key` in the work-group's LDS table (LSLOTS keys, EMPTY = free), -1 when LPROBES probes did not place it
__device__ __forceinline__ int lds_slot(unsigned long long* l_key, unsigned long long key) {
  uint32_t h = hash32(key) & (LSLOTS - 1);
  for (int p = 0; p < LPROBES; ++p) {
    unsigned long long k = l_key[h];
    if (k == EMPTY) {
      k = atomicCAS(&l_key[h], EMPTY, key);
      if (k == EMPTY) k = key;
    }
    if (k == key) return (int)h;
    h = (h + 1) & (LSLOTS - 1);
  }
  return -1;
}

// runs of equal keys along the lanes of a wavefront: `heads` = ballot of "first lane of its run" -> one past the run's last lane
__device__ __forceinline__ int run_end(uint64_t heads, int lane) {
  const uint64_t above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
  return above ? __builtin_ctzll(above) : 64;
}
__device__ __forceinline__ uint64_t lane_range(int from, int to) {  // bits [from, to), to <= 64
  const uint64_t upto = to == 64 ? ~0ull : (1ull << to) - 1ull;
  return upto & ~((1ull << from) - 1ull);
}
// Q quantities per lane, summed over the lanes [lane, end) of the run: the run's first lane ends up with the run's sums
template <int Q>
__device__ __forceinline__ void run_sum(unsigned long long (&v)[Q], int lane, int end) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const unsigned long long o = __shfl_down(v[j], d);
      if (lane + d < end) v[j] += o;
    }
  }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  return v;
}
#endif

}  // namespace swg_pair_table
