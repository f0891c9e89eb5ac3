// The per-genome-pair reduction of the library, defined once.  Its users: swg_alnstats.hip (ordered pairs: bases, matches and
// first record, ALL and KEPT), swg_sparsify.hip (unordered pairs: matches, block length, records) and swg_breadth.hip (ordered
// pairs: bases and union of each axis and first record, ALL and KEPT).  The scheme:
//
//   1. runs of one key along the lanes of a wavefront are summed towards the run's first lane (run_end, run_sum);
//   2. the run heads go through a small LDS table of the work-group (LdsTable); a head that finds no slot there within LPROBES
//      probes is added to the global table directly;
//   3. the LDS table is flushed with one atomic per (work-group, key, quantity) into a global table (PairTable) that is dense
//      (slot = key) while G x G is at most DENSE_LIMIT and open addressing beyond (table_create, table_add);
//   4. the occupied slots are listed with one atomic per wavefront and list (wave_place, list_slots), copied down and, where
//      the table keeps first records, ordered by them (list_fetch).
//
// A kernel keeps its own per-record loop and its own __global__ entry for the listing (the profile's launch labels are kernel
// names); everything it does to a table goes through here.  Integer atomics only.  Below the scheme: what the host entries of
// the three users share (grid_for, share_for, reserve_first).  swg_blocks.hip reduces per chain into a dense table
// of its own and borrows the run and wavefront helpers only.  swg_components.hip keys the same table by SEQUENCE pair: three
// sums (bases of either end, records) and the ALL first record; it lists the slots itself, as swg_link (table_alloc, table_clear).
#pragma once
#include <algorithm>
#include <vector>

#include "swg_internal.h"

namespace swg_pair_table {

constexpr int TB = 256;                    // threads per work-group
constexpr int WAVES = TB / 64;
constexpr int LSLOTS = 256;                // LDS genome-pair slots per work-group
constexpr int LPROBES = 8;                 // ... probed this far, then the run goes to the global table directly
constexpr uint32_t NONE32 = 0xffffffffu;
constexpr unsigned long long EMPTY = ~0ull;
constexpr uint64_t DENSE_LIMIT = uint64_t(1) << 20;  // G * G entries

inline uint64_t pow2_at_least(uint64_t v) {
  uint64_t c = 1024;
  while (c < v) c <<= 1;
  return c;
}

// the slot hash of every open-addressing table here, device and host (a table built on the host is probed on the device)
__host__ __device__ __forceinline__ uint32_t hash32(unsigned long long key) { return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 32); }

// ---- the global table and its listing ------------------------------------------------------------------------------------
// Q u64 sums per slot.  FIRST: also the smallest record index of the slot, ALL and KEPT, and then a row is groups of four sums
// {a ALL, b ALL, a KEPT, b KEPT} (alnstats: one group; breadth: one per axis): the listing has one list per set, an entry of
// which holds the set's two sums of every group.  Without FIRST there is one list of whole rows, and a slot is occupied when
// any of its sums is non-zero (sparsify's record count is one of them).
template <int Q, bool FIRST>
struct PairTable {
  unsigned long long* keys;  // hashed: [mask + 1], EMPTY = free; nullptr = dense (slot = key)
  unsigned long long* sums;  // [slots][Q]
  uint32_t* first;           // FIRST: [slots][2], NONE32 = none
  uint32_t mask;
  uint64_t slots;
};
template <int N, bool FIRST>
struct PairEntry {  // one listed genome pair
  unsigned long long key, v[N], first;
};
template <int N>
struct PairEntry<N, false> {
  unsigned long long key, v[N];
};
template <int Q, bool FIRST>
struct PairList {
  static constexpr int SETS = FIRST ? 2 : 1, N = Q / SETS;
  using Entry = PairEntry<N, FIRST>;
  Entry* out[SETS];           // [cap] each (the KEPT list of a call without a status column: [1], nothing is listed there)
  unsigned long long* count;  // [SETS] among the caller's device scalars, zeroed by the caller
  uint64_t cap;
};

// Sizes the table for G key halves (genomes; sequences for swg_components.hip, whose key is a * n_seq + b) of which at most
// pairs_max pairs occur (hashed: twice the slots of the keys that can occur) and takes it from the running arena frame;
// table_clear, behind the caller's SWG_CHECK_ARENA, clears it on the context's stream.
template <int Q, bool FIRST>
void table_alloc(swg_ctx* ctx, uint32_t G, uint64_t pairs_max, bool force_hash, PairTable<Q, FIRST>* T) {
  const uint64_t g2 = (uint64_t)G * G;
  *T = PairTable<Q, FIRST>{};
  if (g2 <= DENSE_LIMIT && !force_hash) {
    T->slots = g2;
  } else {
    T->slots = pow2_at_least(2 * pairs_max);
    T->mask = (uint32_t)(T->slots - 1);
    T->keys = swg_alloc<unsigned long long>(ctx, T->slots);
  }
  T->sums = swg_alloc<unsigned long long>(ctx, T->slots * Q);
  if (FIRST) T->first = swg_alloc<uint32_t>(ctx, T->slots * 2);
}
template <int Q, bool FIRST>
int table_clear(swg_ctx* ctx, const PairTable<Q, FIRST>& T) {
  hipStream_t st = ctx->stream;
  if (T.keys) SWG_HIP(ctx, hipMemsetAsync(T.keys, 0xff, T.slots * sizeof(unsigned long long), st));
  SWG_HIP(ctx, hipMemsetAsync(T.sums, 0, T.slots * Q * sizeof(unsigned long long), st));
  if (FIRST) SWG_HIP(ctx, hipMemsetAsync(T.first, 0xff, T.slots * 2 * sizeof(uint32_t), st));
  return SWG_OK;
}

// The table with its lists: the genome-pair users' entry.
template <int Q, bool FIRST>
int table_create(swg_ctx* ctx, uint32_t G, uint64_t pairs_max, bool force_hash, bool kept_list, unsigned long long* count,
                 PairTable<Q, FIRST>* T, PairList<Q, FIRST>* L) {
  using Entry = typename PairList<Q, FIRST>::Entry;
  table_alloc(ctx, G, pairs_max, force_hash, T);
  L->cap = pairs_max ? pairs_max : 1;
  L->count = count;
  L->out[0] = swg_alloc<Entry>(ctx, L->cap);
  if (FIRST) L->out[FIRST] = swg_alloc<Entry>(ctx, kept_list ? L->cap : 1);
  SWG_CHECK_ARENA(ctx);
  return table_clear(ctx, *T);
}

// The lists of a table after its listing kernel: `listed` is the host's copy of L.count.  `what` names the caller in the error.
template <int Q, bool FIRST>
int list_fetch(swg_ctx* ctx, const char* what, const PairList<Q, FIRST>& L, const uint64_t* listed,
               std::vector<typename PairList<Q, FIRST>::Entry> (&list)[PairList<Q, FIRST>::SETS]) {
  using Entry = typename PairList<Q, FIRST>::Entry;
  for (int s = 0; s < L.SETS; ++s)
    if (listed[s] > L.cap)
      return swg_set_error(ctx, SWG_ERR_HIP, "%s: internal: %llu genome pairs listed, %llu expected at most", what,
                           (unsigned long long)listed[0], (unsigned long long)L.cap);
  for (int s = 0; s < L.SETS; ++s) {
    list[s].resize(listed[s]);
    if (!list[s].empty())
      SWG_HIP(ctx, hipMemcpyAsync(list[s].data(), L.out[s], list[s].size() * sizeof(Entry), hipMemcpyDeviceToHost, ctx->stream));
  }
  SWG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if constexpr (FIRST)  // (without first records the listing order is whatever the atomics made it)
    for (auto& l : list) std::sort(l.begin(), l.end(), [](const Entry& a, const Entry& b) { return a.first < b.first; });
  return SWG_OK;
}

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

// v[0 .. N) added to the sums [offset, offset + N) of the key's row (the key is inserted when absent); USE_FIRST: the first
// records lowered to f_all and, unless NONE32, f_kept
template <int N, bool USE_FIRST, int Q, bool FIRST>
__device__ __forceinline__ void table_add(const PairTable<Q, FIRST>& T, unsigned long long key, const unsigned long long* v, int offset,
                                          uint32_t f_all = NONE32, uint32_t f_kept = NONE32) {
  static_assert(FIRST || !USE_FIRST, "the table keeps no first records");
  const uint64_t s = T.keys ? table_slot(T.keys, T.mask, key) : key;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (v[j]) atomicAdd(&T.sums[s * Q + offset + j], v[j]);
  if constexpr (USE_FIRST) {
    atomicMin(&T.first[s * 2], f_all);
    if (f_kept != NONE32) atomicMin(&T.first[s * 2 + 1], f_kept);
  }
}

// The work-group's staging table, a __shared__ variable of the kernel: N sums per slot and, with FIRST, the first records.  A
// kernel instance that leaves the first records of its global table alone stages without them (breadth's target axis: the
// query axis has written them).
template <bool FIRST>
struct LdsFirst {
  uint32_t first[LSLOTS][2];
};
template <>
struct LdsFirst<false> {};
template <int N, bool FIRST>
struct LdsTable : LdsFirst<FIRST> {
  unsigned long long key[LSLOTS];
  unsigned long long sum[LSLOTS][N];

  __device__ __forceinline__ void clear() {  // by the whole work-group; a barrier before the first add
    for (int s = threadIdx.x; s < LSLOTS; s += TB) {
      key[s] = EMPTY;
#pragma unroll
      for (int j = 0; j < N; ++j) sum[s][j] = 0;
      if constexpr (FIRST) this->first[s][0] = this->first[s][1] = NONE32;
    }
  }
  // a run head; false when LPROBES probes did not place the key (more keys in this work-group's share than the table takes):
  // the caller adds to the global table
  __device__ __forceinline__ bool add(unsigned long long k, const unsigned long long (&v)[N], uint32_t f_all = NONE32, uint32_t f_kept = NONE32) {
    uint32_t h = hash32(k) & (LSLOTS - 1);
    for (int p = 0; p < LPROBES; ++p, h = (h + 1) & (LSLOTS - 1)) {
      unsigned long long at = key[h];
      if (at == EMPTY) {
        at = atomicCAS(&key[h], EMPTY, k);
        if (at == EMPTY) at = k;
      }
      if (at != k) continue;
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (v[j]) atomicAdd(&sum[h][j], v[j]);
      if constexpr (FIRST) {
        atomicMin(&this->first[h][0], f_all);
        if (f_kept != NONE32) atomicMin(&this->first[h][1], f_kept);
      }
      return true;
    }
    return false;
  }
  // by the whole work-group, after a barrier behind the last add
  template <int Q, bool TABLE_FIRST>
  __device__ __forceinline__ void flush(const PairTable<Q, TABLE_FIRST>& T, int offset) {
    for (int s = threadIdx.x; s < LSLOTS; s += TB) {
      if (key[s] == EMPTY) continue;
      if constexpr (FIRST)
        table_add<N, true>(T, key[s], sum[s], offset, this->first[s][0], this->first[s][1]);
      else
        table_add<N, false>(T, key[s], sum[s], offset);
    }
  }
};

// consecutive places for the lanes of the ballot `m` from one atomic per wavefront
__device__ __forceinline__ unsigned long long wave_place(uint64_t m, unsigned long long* counter) {
  if (!m) return 0;
  const int lane = threadIdx.x & 63;
  unsigned long long base = 0;
  if (lane == __builtin_ctzll(m)) base = atomicAdd(counter, (unsigned long long)__popcll(m));
  base = __shfl(base, __builtin_ctzll(m));
  return base + __popcll(m & ((1ull << lane) - 1ull));
}

// the body of a listing kernel: one lane per slot, launched over T.slots in work-groups of TB
template <int Q, bool FIRST>
__device__ __forceinline__ void list_slots(const PairTable<Q, FIRST>& T, const PairList<Q, FIRST>& L) {
  using List = PairList<Q, FIRST>;
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const bool in = s < T.slots;
  const unsigned long long* row = T.sums + s * Q;
#pragma unroll
  for (int set = 0; set < List::SETS; ++set) {
    uint32_t f = NONE32;
    bool have = false;
    if constexpr (FIRST) {
      if (in) f = T.first[s * 2 + set];
      have = f != NONE32;
    } else if (in) {
#pragma unroll
      for (int j = 0; j < Q; ++j) have |= row[j] != 0;
    }
    const unsigned long long at = wave_place(__ballot(have), &L.count[set]);
    if (have && at < L.cap) {
      typename List::Entry e;
      e.key = T.keys ? T.keys[s] : s;
#pragma unroll
      for (int j = 0; j < List::N; ++j) e.v[j] = FIRST ? row[(j >> 1) * 4 + set * 2 + (j & 1)] : row[j];
      if constexpr (FIRST) e.first = f;
      L.out[set][at] = e;
    }
  }
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

// ---- the host entries ------------------------------------------------------------------------------------------------------
inline unsigned grid_for(const swg_ctx* ctx, uint64_t items) {  // several times the resident work-groups, never more than the work
  const uint64_t tiles = (items + TB - 1) / TB, max_groups = (uint64_t)ctx->num_cu * 8;
  return (unsigned)std::max<uint64_t>(1, std::min(tiles, max_groups));
}

// contiguous shares of n records, whole tiles of TB, one per work-group of a grid_for grid (fewer when the shares round up)
struct Share {
  uint64_t per_group;
  unsigned grid;
};
inline Share share_for(const swg_ctx* ctx, uint64_t n) {
  const uint64_t tiles = (n + TB - 1) / TB, groups = grid_for(ctx, n);
  const uint64_t per_group = (tiles + groups - 1) / groups * TB;
  return Share{per_group, (unsigned)((n + per_group - 1) / per_group)};
}

// a context's first call sizes the arena from its input (later ones grow it on overflow: swg_run_with_arena)
inline int reserve_first(swg_ctx* ctx, size_t want) {
  if (ctx->arena_cap) return SWG_OK;
  return swg_arena_reserve(ctx, std::min(want, swg_arena_budget(ctx)));
}

}  // namespace swg_pair_table
