// Ranged filter: record sets of 2^31 records or more, or whose one-piece footprint does not fit the context's device-memory
// limit (swg_set_memory_limit; no limit: what the device has free), cut into ranges of whole genome pairs (first-two-'#'-parts
// rule).  Genome pairs are the filter's independent units (csrc/host/shard_host.h has the argument), so every range runs the
// unchanged pipeline and the results are those of one call once the chain numbers are made global (csrc/host/range_plan.h).
//
//   device columns (swg_filter_device / swg_filter_device64)
//     plan       range_plan / range_plan_lds: the pair cell of every record -- dense G x G up to 2048 genomes, else the slot of an open-
//                addressing table of the pairs that occur (range_pair_insert) -- and per cell the record count, first and
//                last record and the first record passing the step-1 retain predicate.  Up to 1024 cells a work-group counts
//                its 4096-record tile in LDS and issues one set of atomics per cell it touched; otherwise one set per tile
//                when the tile is one pair (grouped input), one per run of equal pairs inside a thread on mixed tiles.  Only
//                the per-cell arrays come back.
//     pack       host: pairs in first-record order into ranges of at most R records, R from the byte budget
//     per range  a range that is exactly the records [lo, hi) of the caller (pair-major or query-major input) is filtered
//                as a slice of the caller's columns, results written in place; any other range has its record indices
//                listed in ascending order (range_count, range_index: u64), its columns gathered into the context's range
//                block (range_gather) and its results scattered back (range_scatter).  The 64-bit entry rebases the staged
//                (or sliced) range with the existing seq_lo / rebase / axis_* kernels: exact, a range holds whole sweep segments.
//     numbering  range_chain_bounds: every pair's lowest and highest range-local kept chain number; host: shift per pair in
//                order of first retained record; range_chain_shift: one pass over chain_out.
//   host columns (swg_filter / swg_filter_multi): the genome-pair plan of csrc/host/shard_host.h, the same packing, every range
//     gathered through swg_filter_gathered's pinned ring (ranges round-robin over the contexts), results written into the
//     caller's arrays, chain numbers shifted on host threads.  No second copy of the record set on the host.
#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "host/range_plan.h"
#include "host/shard_host.h"
#include "host/stream_plan.h"
#include "swg_internal.h"
#include "swg_pipeline.h"

namespace {

constexpr int EW = 256, PER = 16;
constexpr uint64_t TILE = (uint64_t)EW * PER;
constexpr uint64_t MAX_CELLS = uint64_t(1) << 22;      // dense G x G pair cells up to 2048 genomes; beyond that a hash table
constexpr uint64_t MAX_SLOTS = uint64_t(1) << 24;      // ... of at most 2^24 slots (2^23 genome pairs at half load)
constexpr uint64_t LDS_CELLS = 1024;                   // the plan counts in LDS per work-group up to this many cells
constexpr uint64_t NONE = ~0ull;

inline size_t al(size_t b) { return (b + 255) & ~size_t(255); }

// A record's genome-pair cell: a * G + b for the dense table, else the slot of key a * G + b + 1 in an open-addressing table
// (keys == nullptr: dense)
struct PairMap {
  const uint32_t* g2;
  uint32_t n_seq, G;
  const unsigned long long* keys;
  uint64_t mask;
};
__device__ __forceinline__ uint64_t pair_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return k;
}
__device__ __forceinline__ bool pair_key(uint64_t i, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id, const PairMap& pm,
                                         uint64_t* key) {
  const uint32_t q = q_id[i], t = t_id[i];
  if (q >= pm.n_seq || t >= pm.n_seq) return false;
  const uint32_t a = pm.g2[q], b = pm.g2[t];
  if (a >= pm.G || b >= pm.G) return false;
  *key = (uint64_t)a * pm.G + b;
  return true;
}
__device__ __forceinline__ bool cell_of(uint64_t i, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id, const PairMap& pm,
                                        uint32_t* cell) {
  uint64_t key;
  if (!pair_key(i, q_id, t_id, pm, &key)) return false;
  if (!pm.keys) {
    *cell = (uint32_t)key;
    return true;
  }
  ++key;
  uint64_t h = pair_hash(key) & pm.mask;
  for (uint64_t probe = 0; probe <= pm.mask; ++probe, h = (h + 1) & pm.mask) {
    const unsigned long long k = pm.keys[h];
    if (k == key) {
      *cell = (uint32_t)h;
      return true;
    }
    if (k == 0) return false;
  }
  return false;
}

// the hash table's keys: every distinct pair inserted once (a thread's records are contiguous: runs of one pair probe once)
__global__ __launch_bounds__(256) void range_pair_insert_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                               PairMap pm, unsigned long long* __restrict__ keys,
                                                               unsigned int* __restrict__ overflow) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  uint64_t last = NONE;
  for (int j = 0; j < 16; ++j) {
    const uint64_t i = i0 + j;
    if (i >= n) break;
    uint64_t key;
    if (!pair_key(i, q_id, t_id, pm, &key) || key == last) continue;
    last = key;
    ++key;
    uint64_t h = pair_hash(key) & pm.mask;
    bool placed = false;
    for (uint64_t probe = 0; probe <= pm.mask; ++probe, h = (h + 1) & pm.mask) {
      const unsigned long long old = atomicCAS(&keys[h], 0ull, (unsigned long long)key);
      if (old == 0 || old == key) {
        placed = true;
        break;
      }
    }
    if (!placed) atomicOr(overflow, 1u);
  }
}

// step-1 retain predicate (src/paf_filter.rs:384-388), as shard_host.h make_plan evaluates it
struct RetainArgs {
  uint64_t min_block;
  double min_identity;
  int keep_self;
};
template <class V>
__device__ __forceinline__ bool retained(uint64_t i, const uint32_t* q_id, const uint32_t* t_id, const V* block_len, const V* matches,
                                         const double* identity, const RetainArgs& a) {
  const V b = block_len[i];
  if ((uint64_t)b < a.min_block) return false;
  if (!a.keep_self && q_id[i] == t_id[i]) return false;
  const double id = identity ? identity[i] : (double)matches[i] / (double)(b > 1 ? b : 1);
  return id >= a.min_identity;
}

template <class V>
__global__ __launch_bounds__(EW) void range_plan_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                        PairMap pm, const V* __restrict__ block_len,
                                                        const V* __restrict__ matches, const double* __restrict__ identity, RetainArgs ra,
                                                        unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ first,
                                                        unsigned long long* __restrict__ last, unsigned long long* __restrict__ fret,
                                                        unsigned long long* __restrict__ bad) {
  __shared__ uint32_t s_lo, s_hi;
  __shared__ unsigned long long s_cnt, s_fret;
  const uint64_t base = (uint64_t)blockIdx.x * TILE;
  const uint64_t i0 = base + (uint64_t)threadIdx.x * PER;
  if (threadIdx.x == 0) {
    s_lo = 0xffffffffu;
    s_hi = 0;
    s_cnt = 0;
    s_fret = NONE;
  }
  __syncthreads();
  uint32_t lo = 0xffffffffu, hi = 0;
  for (int j = 0; j < PER; ++j) {
    const uint64_t i = i0 + j;
    if (i >= n) break;
    uint32_t c;
    if (!cell_of(i, q_id, t_id, pm, &c)) {
      atomicMin(bad, (unsigned long long)i);
      lo = 0;  // (never one pair: the tile takes the per-run path, which skips the record)
      hi = 0xffffffffu;
      continue;
    }
    lo = c < lo ? c : lo;
    hi = c > hi ? c : hi;
  }
  if (lo <= hi) {
    atomicMin(&s_lo, lo);
    atomicMax(&s_hi, hi);
  }
  __syncthreads();
  if (s_lo == s_hi) {  // the whole tile is one pair: one set of atomics for the work-group
    unsigned long long c = 0, f = NONE;
    for (int j = 0; j < PER; ++j) {
      const uint64_t i = i0 + j;
      if (i >= n) break;
      ++c;
      if (f == NONE && retained(i, q_id, t_id, block_len, matches, identity, ra)) f = i;
    }
    if (c) atomicAdd(&s_cnt, c);
    if (f != NONE) atomicMin(&s_fret, f);
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t cell = s_lo;
      const uint64_t end = base + TILE < n ? base + TILE : n;
      atomicAdd(&cnt[cell], s_cnt);
      atomicMin(&first[cell], (unsigned long long)base);
      atomicMax(&last[cell], (unsigned long long)(end - 1));
      if (s_fret != NONE) atomicMin(&fret[cell], s_fret);
    }
    return;
  }
  uint32_t rc = 0xffffffffu;
  unsigned long long rn = 0, rf = 0, rl = 0, rr = NONE;
  auto flush = [&]() {
    if (!rn) return;
    atomicAdd(&cnt[rc], rn);
    atomicMin(&first[rc], rf);
    atomicMax(&last[rc], rl);
    if (rr != NONE) atomicMin(&fret[rc], rr);
  };
  for (int j = 0; j < PER; ++j) {
    const uint64_t i = i0 + j;
    if (i >= n) break;
    uint32_t c;
    if (!cell_of(i, q_id, t_id, pm, &c)) continue;
    if (c != rc) {
      flush();
      rc = c;
      rn = 0;
      rf = i;
      rr = NONE;
    }
    ++rn;
    rl = i;
    if (rr == NONE && retained(i, q_id, t_id, block_len, matches, identity, ra)) rr = i;
  }
  flush();
}

// The same counts when the cells fit LDS: a work-group accumulates its tile there and then issues one set of atomics per cell
// it touched, whatever the order of the records (shuffled input over few genomes)
template <class V>
__global__ __launch_bounds__(EW) void range_plan_lds_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                            PairMap pm, const V* __restrict__ block_len, const V* __restrict__ matches,
                                                            const double* __restrict__ identity, RetainArgs ra, uint32_t cells,
                                                            unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ first,
                                                            unsigned long long* __restrict__ last, unsigned long long* __restrict__ fret,
                                                            unsigned long long* __restrict__ bad) {
  __shared__ uint32_t s_cnt[LDS_CELLS];
  __shared__ unsigned long long s_first[LDS_CELLS], s_last[LDS_CELLS], s_fret[LDS_CELLS];
  for (uint32_t c = threadIdx.x; c < cells; c += EW) {
    s_cnt[c] = 0;
    s_first[c] = NONE;
    s_last[c] = 0;
    s_fret[c] = NONE;
  }
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * PER;
  uint32_t rc = 0xffffffffu, rn = 0;
  unsigned long long rf = 0, rl = 0, rr = NONE;
  auto flush = [&]() {
    if (!rn) return;
    atomicAdd(&s_cnt[rc], rn);
    atomicMin(&s_first[rc], rf);
    atomicMax(&s_last[rc], rl);
    if (rr != NONE) atomicMin(&s_fret[rc], rr);
  };
  for (int j = 0; j < PER; ++j) {
    const uint64_t i = i0 + j;
    if (i >= n) break;
    uint32_t c;
    if (!cell_of(i, q_id, t_id, pm, &c) || c >= cells) {
      atomicMin(bad, (unsigned long long)i);
      continue;
    }
    if (c != rc) {
      flush();
      rc = c;
      rn = 0;
      rf = i;
      rr = NONE;
    }
    ++rn;
    rl = i;
    if (rr == NONE && retained(i, q_id, t_id, block_len, matches, identity, ra)) rr = i;
  }
  flush();
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < cells; c += EW)
    if (s_cnt[c]) {
      atomicAdd(&cnt[c], (unsigned long long)s_cnt[c]);
      atomicMin(&first[c], s_first[c]);
      atomicMax(&last[c], s_last[c]);
      if (s_fret[c] != NONE) atomicMin(&fret[c], s_fret[c]);
    }
}

// records of range k per tile of TILE records
__global__ __launch_bounds__(EW) void range_count_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                         PairMap pm,
                                                         const uint32_t* __restrict__ range_of, uint32_t k, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t s;
  if (threadIdx.x == 0) s = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * PER;
  uint32_t c = 0;
  for (int j = 0; j < PER; ++j) {
    const uint64_t i = i0 + j;
    if (i >= n) break;
    uint32_t cell;
    if (cell_of(i, q_id, t_id, pm, &cell) && range_of[cell] == k) ++c;
  }
  if (c) atomicAdd(&s, c);
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s;
}

// the record indices of range k, ascending: tile_off = exclusive sum of range_count's tile counts
__global__ __launch_bounds__(EW) void range_index_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                         PairMap pm,
                                                         const uint32_t* __restrict__ range_of, uint32_t k,
                                                         const unsigned long long* __restrict__ tile_off, unsigned long long* __restrict__ idx) {
  __shared__ uint32_t pre[EW];
  const uint64_t i0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * PER;
  uint32_t mask = 0;
  for (int j = 0; j < PER; ++j) {
    const uint64_t i = i0 + j;
    if (i >= n) break;
    uint32_t cell;
    if (cell_of(i, q_id, t_id, pm, &cell) && range_of[cell] == k) mask |= 1u << j;
  }
  const uint32_t mine = (uint32_t)__popc(mask);
  pre[threadIdx.x] = mine;
  __syncthreads();
  for (int d = 1; d < EW; d <<= 1) {  // inclusive scan over the work-group
    const uint32_t v = threadIdx.x >= (unsigned)d ? pre[threadIdx.x - d] : 0;
    __syncthreads();
    pre[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned long long pos = tile_off[blockIdx.x] + (pre[threadIdx.x] - mine);
  for (int j = 0; j < PER; ++j)
    if (mask & (1u << j)) idx[pos++] = i0 + j;
}

template <class V>
struct Cols {
  const uint32_t* q_id;
  const uint32_t* t_id;
  const V* c[6];  // q_start q_end t_start t_end matches block_len
  const double* identity;
  const uint8_t* strand;
};
template <class V>
struct OutCols {
  uint32_t* q_id;
  uint32_t* t_id;
  V* c[6];
  double* identity;
  uint8_t* strand;
};

template <class V>
__global__ __launch_bounds__(EW) void range_gather_kernel(uint64_t m, const unsigned long long* __restrict__ idx, Cols<V> s, OutCols<V> d) {
  const uint64_t j = (uint64_t)blockIdx.x * EW + threadIdx.x;
  if (j >= m) return;
  const uint64_t i = idx[j];
  d.q_id[j] = s.q_id[i];
  d.t_id[j] = s.t_id[i];
#pragma unroll
  for (int c = 0; c < 6; ++c) d.c[c][j] = s.c[c][i];
  if (s.identity) d.identity[j] = s.identity[i];
  d.strand[j] = s.strand[i];
}

__global__ __launch_bounds__(EW) void range_scatter_kernel(uint64_t m, const unsigned long long* __restrict__ idx, const uint8_t* __restrict__ st,
                                                           const uint32_t* __restrict__ ch, uint8_t* __restrict__ status_out,
                                                           uint32_t* __restrict__ chain_out) {
  const uint64_t j = (uint64_t)blockIdx.x * EW + threadIdx.x;
  if (j >= m) return;
  const uint64_t i = idx[j];
  status_out[i] = st[j];
  chain_out[i] = ch[j];
}

// lowest / highest non-zero chain number per pair cell over one range's results
__global__ __launch_bounds__(EW) void range_chain_bounds_kernel(uint64_t m, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                                PairMap pm,
                                                                const uint32_t* __restrict__ chain, uint32_t* __restrict__ lo,
                                                                uint32_t* __restrict__ hi) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * EW + threadIdx.x) * PER;
  uint32_t rc = 0xffffffffu, rlo = 0xffffffffu, rhi = 0;
  for (int j = 0; j < PER; ++j) {
    const uint64_t i = i0 + j;
    if (i >= m) break;
    const uint32_t c = chain[i];
    uint32_t cell;
    if (!c || !cell_of(i, q_id, t_id, pm, &cell)) continue;
    if (cell != rc) {
      if (rhi) {
        atomicMin(&lo[rc], rlo);
        atomicMax(&hi[rc], rhi);
      }
      rc = cell;
      rlo = 0xffffffffu;
      rhi = 0;
    }
    rlo = c < rlo ? c : rlo;
    rhi = c > rhi ? c : rhi;
  }
  if (rhi) {
    atomicMin(&lo[rc], rlo);
    atomicMax(&hi[rc], rhi);
  }
}

__global__ __launch_bounds__(EW) void range_chain_shift_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                               PairMap pm,
                                                               const long long* __restrict__ shift, uint32_t* __restrict__ chain) {
  const uint64_t i = (uint64_t)blockIdx.x * EW + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = chain[i];
  uint32_t cell;
  if (c && cell_of(i, q_id, t_id, pm, &cell)) chain[i] = (uint32_t)((long long)c + shift[cell]);
}

inline unsigned blocks(uint64_t n, uint64_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// device bytes of one gathered range of m records: indices, staged columns (value columns of `vw` bytes), status, chain
size_t stage_bytes(uint64_t m, size_t vw) {
  return al(m * 8) + 2 * al(m * 4) + 6 * al(m * vw) + al(m * 8) + al(m) + al(m) + al(m * 4);
}

int range_block_reserve(swg_ctx* ctx, size_t bytes) {
  // (under a limit the block is exactly this call's size: a larger one left by an earlier call would take the arena's share)
  if (ctx->range_cap >= bytes && (!ctx->mem_limit || ctx->range_cap == bytes)) return SWG_OK;
  SWG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->range_block) {
    SWG_HIP(ctx, hipFree(ctx->range_block));
    ctx->range_block = nullptr;
    ctx->range_cap = 0;
  }
  if (ctx->mem_limit) {
    if ((uint64_t)bytes + ctx->io_cap > ctx->mem_limit)
      return swg_set_error(ctx, SWG_ERR_OOM, "%zu bytes of range staging do not fit the memory limit of %llu bytes", bytes,
                           (unsigned long long)ctx->mem_limit);
    if ((uint64_t)bytes + ctx->io_cap + ctx->arena_cap > ctx->mem_limit && ctx->arena) {
      SWG_HIP(ctx, hipFree(ctx->arena));
      ctx->arena = nullptr;
      ctx->arena_cap = 0;
    }
  }
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess)
    return swg_set_error(ctx, SWG_ERR_OOM, "hipMalloc of %zu bytes for range staging failed: %s", bytes, hipGetErrorString(e));
  ctx->range_block = static_cast<char*>(p);
  ctx->range_cap = bytes;
  return SWG_OK;
}

// bytes one call may still take on this context's device: the limit beside what other calls' blocks hold, or (no limit)
// what is free plus what the context's own blocks would give back
uint64_t device_budget(swg_ctx* ctx, bool host_staging) {
  if (ctx->mem_limit) {
    const uint64_t held = host_staging ? ctx->range_cap : ctx->io_cap;
    return held < ctx->mem_limit ? ctx->mem_limit - held : 0;
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
  const uint64_t have = (uint64_t)free_b + ctx->arena_cap + (host_staging ? ctx->io_cap : ctx->range_cap);
  // (a quarter held back: the runtime's own allocations, fragmentation, and room for a range whose scratch outgrows its budget)
  const uint64_t margin = std::max<uint64_t>(uint64_t(256) << 20, have / 4);
  return have > margin ? have - margin : 0;
}

void add_stats(swg_stats* acc, const swg_stats& a) {
  acc->n_retained += a.n_retained;
  acc->n_swept += a.n_swept;
  acc->n_chains += a.n_chains;
  acc->n_chains_kept += a.n_chains_kept;
  acc->n_out += a.n_out;
}

// what an oversize pair did not fit, for its error message
std::string what_bounds(const swg_ctx* ctx) {
  if (!ctx->mem_limit) return "the device's free memory";
  return "the device memory limit of " + std::to_string((unsigned long long)ctx->mem_limit) + " bytes";
}

const char* const UNSUPPORTED_PREFIX =
    "the two genome-prefix rules (last '#', first two '#' parts) partition the sequences differently: a record set of 2^31 records "
    "or more, or beyond the device-memory limit, is filtered in ranges of whole genome pairs, which needs them to agree";

}  // namespace

int swg_device_needs_ranges(swg_ctx* ctx, const swg_records* rec, const swg_config* cfg, bool wide, bool* ranged) {
  *ranged = false;
  const uint64_t n = rec->n;
  if (n == 0) return SWG_OK;
  if (n > swg_range::MAX_RANGE) {
    *ranged = true;
    return SWG_OK;
  }
  const uint64_t est = swg_arena_estimate(n, rec, cfg, wide);
  if (ctx->mem_limit) {
    *ranged = est > swg_arena_budget(ctx);
    return SWG_OK;
  }
  if (est <= ctx->arena_cap) return SWG_OK;  // (steady state: no query)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return SWG_OK;  // unknown: one piece, as always
  *ranged = est > (uint64_t)free_b + ctx->arena_cap + ctx->range_cap;  // (what the context's own blocks hold is available too)
  return SWG_OK;
}

int swg_host_needs_ranges(swg_ctx* const* ctxs, int n_ctx, const swg_records* rec, const swg_config* cfg, bool* ranged) {
  *ranged = false;
  const uint64_t n = rec->n;
  if (n == 0) return SWG_OK;
  if (n > swg_range::MAX_RANGE) {
    *ranged = true;
    return SWG_OK;
  }
  const uint64_t one_piece = swg_io_block_bytes(n, rec->n_seq) + swg_arena_estimate(n, rec, cfg, false);
  for (int d = 0; d < n_ctx; ++d) {
    swg_ctx* ctx = ctxs[d];
    if (ctx->mem_limit) {
      if (one_piece + ctx->range_cap > ctx->mem_limit) *ranged = true;
    } else if (n_ctx == 1 && one_piece > (uint64_t)ctx->arena_cap + ctx->io_cap) {
      SWG_HIP(ctx, hipSetDevice(ctx->device));
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && one_piece > (uint64_t)free_b + ctx->arena_cap + ctx->io_cap) *ranged = true;
    }
  }
  return SWG_OK;
}

// ---- device columns -------------------------------------------------------------------------------------------------------
int swg_filter_ranged_device(swg_ctx* ctx, const swg_records* rec, const swg_records64* rec64, const swg_config* cfg, uint8_t* status_out,
                             uint32_t* chain_out, swg_stats* stats) {
  const uint64_t n = rec->n;
  const bool wide = rec64 != nullptr;
  const size_t vw = wide ? 8 : 4;
  hipStream_t st = ctx->stream;
  const uint32_t ns = rec->n_seq, G = rec->n_genome_two;
  // the two genome tables on the host: both prefix rules must give the same genomes
  std::vector<uint32_t> hgl(ns), hg2(ns);
  SWG_HIP(ctx, hipMemcpyAsync(hgl.data(), rec->seq_genome_last, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
  SWG_HIP(ctx, hipMemcpyAsync(hg2.data(), rec->seq_genome_two, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
  SWG_HIP(ctx, hipStreamSynchronize(st));
  {
    swg_records hv = *rec;
    hv.seq_genome_last = hgl.data();
    hv.seq_genome_two = hg2.data();
    if (!swg_streamed::same_partition(&hv)) return swg_set_error(ctx, SWG_ERR_UNSUPPORTED, "%s", UNSUPPORTED_PREFIX);
  }
  // genome-pair cells: dense G x G up to 2048 genomes (names without '#': every sequence its own genome), else a hash table
  // over the pairs that occur, of at least twice their possible number (at most min(n, G^2)) slots
  const bool hashed = (uint64_t)G * G > MAX_CELLS;
  uint64_t cells = (uint64_t)G * G;
  if (hashed) {
    const uint64_t bound = std::min<uint64_t>(n, (uint64_t)G * G);
    cells = 1024;
    while (cells < 2 * bound && cells < MAX_SLOTS) cells <<= 1;
  }
  PairMap pm{rec->seq_genome_two, ns, G, nullptr, cells - 1};
  std::vector<unsigned long long> keys(hashed ? cells : 0);
  const uint64_t tiles = (n + TILE - 1) / TILE;

  // ---- plan: per-cell counts (and the hash table's keys) in the arena, copied back
  std::vector<uint64_t> cnt(cells), first(cells), last(cells), fret(cells);
  uint64_t bad = NONE;
  unsigned int overflow = 0;
  {
    const size_t want = (hashed ? 5 : 4) * al(cells * 8) + 512;
    if (ctx->arena_cap < want) SWG_TRY(swg_arena_reserve(ctx, want));
    SWG_TRY(swg_run_with_arena(ctx, [&]() -> int {
      unsigned long long* a = swg_alloc<unsigned long long>(ctx, 4 * cells + 1);
      unsigned long long* d_keys = hashed ? swg_alloc<unsigned long long>(ctx, cells + 1) : nullptr;
      SWG_CHECK_ARENA(ctx);
      unsigned long long *d_cnt = a, *d_first = a + cells, *d_last = a + 2 * cells, *d_fret = a + 3 * cells, *d_bad = a + 4 * cells;
      if (hashed) {
        unsigned int* d_over = reinterpret_cast<unsigned int*>(d_keys + cells);
        SWG_HIP(ctx, hipMemsetAsync(d_keys, 0, (cells + 1) * 8, st));
        SWG_LAUNCH(ctx, "range_pair_insert", range_pair_insert_kernel<<<blocks(n, TILE), 256, 0, st>>>(n, rec->q_id, rec->t_id, pm, d_keys, d_over));
        SWG_KERNEL_CHECK(ctx);
        SWG_HIP(ctx, hipMemcpyAsync(keys.data(), d_keys, cells * 8, hipMemcpyDeviceToHost, st));
        SWG_HIP(ctx, hipMemcpyAsync(&overflow, d_over, 4, hipMemcpyDeviceToHost, st));
        pm.keys = d_keys;
      }
      SWG_HIP(ctx, hipMemsetAsync(d_cnt, 0, cells * 8, st));
      SWG_HIP(ctx, hipMemsetAsync(d_first, 0xff, cells * 8, st));
      SWG_HIP(ctx, hipMemsetAsync(d_last, 0, cells * 8, st));
      SWG_HIP(ctx, hipMemsetAsync(d_fret, 0xff, (cells + 1) * 8, st));  // (and the error word)
      const RetainArgs ra{cfg->min_block_length, cfg->min_identity, cfg->keep_self};
      const bool lds = cells <= LDS_CELLS;
      if (wide && lds)
        SWG_LAUNCH(ctx, "range_plan_lds", range_plan_lds_kernel<uint64_t><<<blocks(n, TILE), EW, 0, st>>>(n, rec->q_id, rec->t_id, pm,
                                                                                                     rec64->block_len, rec64->matches, rec->identity, ra,
                                                                                                     (uint32_t)cells, d_cnt, d_first, d_last, d_fret, d_bad));
      else if (lds)
        SWG_LAUNCH(ctx, "range_plan_lds", range_plan_lds_kernel<uint32_t><<<blocks(n, TILE), EW, 0, st>>>(n, rec->q_id, rec->t_id, pm,
                                                                                                     rec->block_len, rec->matches, rec->identity, ra,
                                                                                                     (uint32_t)cells, d_cnt, d_first, d_last, d_fret, d_bad));
      else if (wide)
        SWG_LAUNCH(ctx, "range_plan", range_plan_kernel<uint64_t><<<blocks(n, TILE), EW, 0, st>>>(n, rec->q_id, rec->t_id, pm,
                                                                                                 rec64->block_len, rec64->matches, rec->identity, ra,
                                                                                                 d_cnt, d_first, d_last, d_fret, d_bad));
      else
        SWG_LAUNCH(ctx, "range_plan", range_plan_kernel<uint32_t><<<blocks(n, TILE), EW, 0, st>>>(n, rec->q_id, rec->t_id, pm,
                                                                                                 rec->block_len, rec->matches, rec->identity, ra,
                                                                                                 d_cnt, d_first, d_last, d_fret, d_bad));
      SWG_KERNEL_CHECK(ctx);
      SWG_HIP(ctx, hipMemcpyAsync(cnt.data(), d_cnt, cells * 8, hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipMemcpyAsync(first.data(), d_first, cells * 8, hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipMemcpyAsync(last.data(), d_last, cells * 8, hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipMemcpyAsync(fret.data(), d_fret, cells * 8, hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));
      return SWG_OK;
    }));
  }
  if (overflow)
    return swg_set_error(ctx, SWG_ERR_UNSUPPORTED, "more than %llu distinct genome pairs: beyond the ranged filter's pair table",
                         (unsigned long long)(MAX_SLOTS / 2));
  if (bad != NONE) return swg_set_error(ctx, SWG_ERR_INVALID, "record %llu: sequence id or genome id out of range", (unsigned long long)bad);

  // ---- pack: R from the budget (the fixed part: per-cell range ids, chain bounds and shifts, the tile counts and offsets)
  const size_t fixed = 3 * al(cells * 4) + al(cells * 8) + al(tiles * 4) + al(tiles * 8) + (hashed ? al(cells * 8) : 0);
  const uint64_t budget = device_budget(ctx, false);
  const uint64_t R = budget > fixed ? swg_range::largest(swg_range::MAX_RANGE, budget - fixed, [&](uint64_t m) {
    return (uint64_t)stage_bytes(m, vw) + swg_arena_estimate(m, rec, cfg, wide);
  }) : 0;
  if (R == 0)
    return swg_set_error(ctx, SWG_ERR_OOM, "the ranged filter needs more than the %llu bytes of device memory %s", (unsigned long long)budget,
                         ctx->mem_limit ? "the memory limit leaves" : "that are free");
  std::vector<swg_range::Range> ranges;
  std::vector<uint32_t> range_of(cells);
  uint32_t badp = 0;
  if (swg_range::pack((uint32_t)cells, cnt.data(), first.data(), last.data(), R, &ranges, range_of.data(), &badp) != swg_range::PACK_OK)
  {
    const uint64_t key = hashed ? keys[badp] - 1 : badp;
    return swg_set_error(ctx, SWG_ERR_RANGE, "genome pair (%llu, %llu) has %llu records: 2^31 or more records in one genome pair are not supported",
                         (unsigned long long)(key / G), (unsigned long long)(key % G), (unsigned long long)cnt[badp]);
  }
  uint64_t m_stage = 0;  // staging for the largest range that is gathered (contiguous ranges are slices of the caller's columns)
  for (const auto& g : ranges)
    if (!g.contiguous) m_stage = std::max(m_stage, g.count);
  const size_t stage = m_stage ? stage_bytes(m_stage, vw) : 0;
  {
    const int rc = range_block_reserve(ctx, fixed + stage);
    if (rc != SWG_OK) {
      if (rc != SWG_ERR_OOM) return rc;
      uint64_t big = 0;
      for (const auto& g : ranges)
        if (g.oversize && !g.contiguous) big = std::max(big, g.count);
      if (!big) return rc;
      const std::string msg = swg_last_error(ctx);
      return swg_set_error(ctx, SWG_ERR_OOM, "a genome pair of %llu records does not fit %s (%s)",
                           (unsigned long long)big, what_bounds(ctx).c_str(), msg.c_str());
    }
  }
  char* blk = ctx->range_block;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = blk + off;
    off += al(bytes);
    return p;
  };
  uint32_t* d_range_of = reinterpret_cast<uint32_t*>(take(cells * 4));
  uint32_t* d_lo = reinterpret_cast<uint32_t*>(take(cells * 4));
  uint32_t* d_hi = reinterpret_cast<uint32_t*>(take(cells * 4));
  long long* d_shift = reinterpret_cast<long long*>(take(cells * 8));
  uint32_t* d_tile_cnt = reinterpret_cast<uint32_t*>(take(tiles * 4));
  unsigned long long* d_tile_off = reinterpret_cast<unsigned long long*>(take(tiles * 8));
  if (hashed) {  // the table's keys for the passes below
    unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(take(cells * 8));
    SWG_HIP(ctx, hipMemcpyAsync(d_keys, keys.data(), cells * 8, hipMemcpyHostToDevice, st));
    pm.keys = d_keys;
  }
  const size_t stage_off = off;
  SWG_HIP(ctx, hipMemcpyAsync(d_range_of, range_of.data(), cells * 4, hipMemcpyHostToDevice, st));
  SWG_HIP(ctx, hipMemsetAsync(d_lo, 0xff, cells * 4, st));
  SWG_HIP(ctx, hipMemsetAsync(d_hi, 0, cells * 4, st));
  static const bool dbg = getenv("SWG_DEBUG") != nullptr;
  if (dbg) fprintf(stderr, "[swg] ranged device call over %llu records: %zu ranges of at most %llu records (budget %llu bytes)\n",
                   (unsigned long long)n, ranges.size(), (unsigned long long)R, (unsigned long long)budget);

  swg_stats acc{};
  std::vector<uint32_t> h_tile(tiles);
  std::vector<uint64_t> h_off(tiles);
  for (size_t k = 0; k < ranges.size(); ++k) {
    const swg_range::Range& g = ranges[k];
    const uint64_t m = g.count;
    swg_records sub = *rec;
    swg_records64 sub64 = rec64 ? *rec64 : swg_records64{};
    sub.n = sub64.n = m;
    uint8_t* st_out;
    uint32_t* ch_out;
    unsigned long long* d_idx = nullptr;
    if (g.contiguous) {  // a slice of the caller's columns, results in place
      const uint64_t lo = g.lo;
      sub.q_id = rec->q_id + lo;
      sub.t_id = rec->t_id + lo;
      sub.identity = rec->identity ? rec->identity + lo : nullptr;
      sub.strand = rec->strand + lo;
      if (wide) {
        sub64.q_id = sub.q_id;
        sub64.t_id = sub.t_id;
        sub64.identity = sub.identity;
        sub64.strand = sub.strand;
        sub64.q_start = rec64->q_start + lo; sub64.q_end = rec64->q_end + lo; sub64.t_start = rec64->t_start + lo; sub64.t_end = rec64->t_end + lo;
        sub64.matches = rec64->matches + lo; sub64.block_len = rec64->block_len + lo;
      } else {
        sub.q_start = rec->q_start + lo; sub.q_end = rec->q_end + lo; sub.t_start = rec->t_start + lo; sub.t_end = rec->t_end + lo;
        sub.matches = rec->matches + lo; sub.block_len = rec->block_len + lo;
      }
      st_out = status_out + lo;
      ch_out = chain_out + lo;
    } else {
      // the range's record indices (ascending), then its columns
      SWG_LAUNCH(ctx, "range_count", range_count_kernel<<<(unsigned)tiles, EW, 0, st>>>(n, rec->q_id, rec->t_id, pm,
                                                                                     d_range_of, (uint32_t)k, d_tile_cnt));
      SWG_KERNEL_CHECK(ctx);
      SWG_HIP(ctx, hipMemcpyAsync(h_tile.data(), d_tile_cnt, tiles * 4, hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));
      uint64_t acc_off = 0;
      for (uint64_t t = 0; t < tiles; ++t) {
        h_off[t] = acc_off;
        acc_off += h_tile[t];
      }
      if (acc_off != m) return swg_set_error(ctx, SWG_ERR_HIP, "range %zu: %llu records listed, %llu planned", k, (unsigned long long)acc_off,
                                             (unsigned long long)m);
      SWG_HIP(ctx, hipMemcpyAsync(d_tile_off, h_off.data(), tiles * 8, hipMemcpyHostToDevice, st));
      off = stage_off;
      d_idx = reinterpret_cast<unsigned long long*>(take(m * 8));
      SWG_LAUNCH(ctx, "range_index", range_index_kernel<<<(unsigned)tiles, EW, 0, st>>>(n, rec->q_id, rec->t_id, pm,
                                                                                     d_range_of, (uint32_t)k, d_tile_off, d_idx));
      SWG_KERNEL_CHECK(ctx);
      uint32_t* q = reinterpret_cast<uint32_t*>(take(m * 4));
      uint32_t* t = reinterpret_cast<uint32_t*>(take(m * 4));
      char* c[6];
      for (auto& p : c) p = take(m * vw);
      double* idn = reinterpret_cast<double*>(take(m * 8));
      uint8_t* sd = reinterpret_cast<uint8_t*>(take(m));
      st_out = reinterpret_cast<uint8_t*>(take(m));
      ch_out = reinterpret_cast<uint32_t*>(take(m * 4));
      if (off > ctx->range_cap) return swg_set_error(ctx, SWG_ERR_HIP, "range staging overrun (%zu > %zu bytes)", off, ctx->range_cap);
      sub.q_id = q;
      sub.t_id = t;
      sub.identity = rec->identity ? idn : nullptr;
      sub.strand = sd;
      if (wide) {
        Cols<uint64_t> s{rec->q_id, rec->t_id, {rec64->q_start, rec64->q_end, rec64->t_start, rec64->t_end, rec64->matches, rec64->block_len},
                         rec->identity, rec->strand};
        OutCols<uint64_t> d{q, t, {}, idn, sd};
        for (int j = 0; j < 6; ++j) d.c[j] = reinterpret_cast<uint64_t*>(c[j]);
        SWG_LAUNCH(ctx, "range_gather", range_gather_kernel<uint64_t><<<blocks(m, EW), EW, 0, st>>>(m, d_idx, s, d));
        sub64.q_id = q;
        sub64.t_id = t;
        sub64.identity = sub.identity;
        sub64.strand = sd;
        sub64.q_start = d.c[0]; sub64.q_end = d.c[1]; sub64.t_start = d.c[2]; sub64.t_end = d.c[3]; sub64.matches = d.c[4]; sub64.block_len = d.c[5];
      } else {
        Cols<uint32_t> s{rec->q_id, rec->t_id, {rec->q_start, rec->q_end, rec->t_start, rec->t_end, rec->matches, rec->block_len},
                         rec->identity, rec->strand};
        OutCols<uint32_t> d{q, t, {}, idn, sd};
        for (int j = 0; j < 6; ++j) d.c[j] = reinterpret_cast<uint32_t*>(c[j]);
        SWG_LAUNCH(ctx, "range_gather", range_gather_kernel<uint32_t><<<blocks(m, EW), EW, 0, st>>>(m, d_idx, s, d));
        sub.q_start = d.c[0]; sub.q_end = d.c[1]; sub.t_start = d.c[2]; sub.t_end = d.c[3]; sub.matches = d.c[4]; sub.block_len = d.c[5];
      }
      SWG_KERNEL_CHECK(ctx);
    }
    // the range through the unchanged pipeline
    swg_stats rs{};
    SWG_TRY(swg_filter_reserve_arena(ctx, m, &sub, cfg, wide));
    int rc = swg_run_with_arena(ctx, [&]() -> int { return swg_filter_piece(ctx, &sub, wide ? &sub64 : nullptr, cfg, st_out, ch_out, &rs); });
    if (rc == SWG_ERR_OOM && g.oversize) {
      const std::string msg = swg_last_error(ctx);
      return swg_set_error(ctx, SWG_ERR_OOM, "a genome pair of %llu records does not fit %s (%s)",
                           (unsigned long long)m, what_bounds(ctx).c_str(), msg.c_str());
    }
    if (rc != SWG_OK) return rc;
    add_stats(&acc, rs);
    SWG_LAUNCH_N(ctx, "range_chain_bounds", m, range_chain_bounds_kernel<<<blocks(m, (uint64_t)EW * PER), EW, 0, st>>>(m, sub.q_id, sub.t_id, pm, ch_out, d_lo, d_hi));
    SWG_KERNEL_CHECK(ctx);
    if (!g.contiguous) {
      SWG_LAUNCH(ctx, "range_scatter", range_scatter_kernel<<<blocks(m, EW), EW, 0, st>>>(m, d_idx, st_out, ch_out, status_out, chain_out));
      SWG_KERNEL_CHECK(ctx);
    }
  }

  // ---- global chain numbers: shift per pair, one pass
  if (cfg->scaffold_gap != 0) {
    std::vector<uint32_t> lo(cells), hi(cells);
    SWG_HIP(ctx, hipMemcpyAsync(lo.data(), d_lo, cells * 4, hipMemcpyDeviceToHost, st));
    SWG_HIP(ctx, hipMemcpyAsync(hi.data(), d_hi, cells * 4, hipMemcpyDeviceToHost, st));
    SWG_HIP(ctx, hipStreamSynchronize(st));
    std::vector<int64_t> shift(cells);
    uint64_t total = 0;
    if (!swg_range::shifts((uint32_t)cells, lo.data(), hi.data(), fret.data(), shift.data(), &total))
      return swg_set_error(ctx, SWG_ERR_RANGE, "%llu kept chains: chain numbers of 2^32 or more are not supported", (unsigned long long)total);
    bool any = false;
    for (int64_t s : shift) any = any || s != 0;
    if (any) {
      SWG_HIP(ctx, hipMemcpyAsync(d_shift, shift.data(), cells * 8, hipMemcpyHostToDevice, st));
      SWG_LAUNCH(ctx, "range_chain_shift", range_chain_shift_kernel<<<blocks(n, EW), EW, 0, st>>>(n, rec->q_id, rec->t_id, pm,
                                                                                                 d_shift, chain_out));
      SWG_KERNEL_CHECK(ctx);
    }
    // (the host vectors above are read by asynchronous copies: wait for them before they go out of scope)
    SWG_HIP(ctx, hipStreamSynchronize(st));
  }
  if (!ctx->mem_limit && ctx->range_block) {
    // no limit: the staging block goes back to the device (tens of GB at 2^31 records); a later call of ordinary size must not
    // find the device full of this context's own memory
    SWG_HIP(ctx, hipStreamSynchronize(st));
    SWG_HIP(ctx, hipFree(ctx->range_block));
    ctx->range_block = nullptr;
    ctx->range_cap = 0;
  }
  if (stats) {
    *stats = acc;
    stats->n_in = n;
  }
  return SWG_OK;
}

// ---- host columns ---------------------------------------------------------------------------------------------------------
int swg_filter_ranged_host(swg_ctx* const* ctxs, int n_ctx, const swg_records* rec, const swg_config* cfg, uint8_t* status_out,
                           uint32_t* chain_out, swg_stats* stats) {
  swg_ctx* ctx0 = ctxs[0];
  const uint64_t n = rec->n;
  if (!swg_streamed::same_partition(rec)) return swg_set_error(ctx0, SWG_ERR_UNSUPPORTED, "%s", UNSUPPORTED_PREFIX);
  swg_shard::Plan P;
  std::vector<swg_range::Range> ranges;
  std::vector<uint32_t> range_of;
  std::vector<uint64_t> first, last;
  uint64_t R = swg_range::MAX_RANGE;
  const int threads = swg_shard::default_threads(n);
  try {
    if (!swg_shard::make_plan(*rec, *cfg, 1, threads, &P))
      return swg_set_error(ctx0, SWG_ERR_INVALID, "sequence id out of range (record %llu)", (unsigned long long)P.bad_record);
    const uint32_t np = P.n_pairs;
    // first / last record of every pair (pair ids are in order of first appearance)
    std::vector<std::vector<uint64_t>> ft(threads), lt(threads);
    swg_host::run(P.threads, [&](int t) {
      ft[t].assign(np, NONE);
      lt[t].assign(np, 0);
      const uint64_t b = n * (uint64_t)t / P.threads, e = n * (uint64_t)(t + 1) / P.threads;
      const uint32_t* pair = P.pair.data();
      for (uint64_t i = b; i < e; ++i) {
        const uint32_t p = pair[i];
        if (ft[t][p] == NONE) ft[t][p] = i;
        lt[t][p] = i;
      }
    });
    first.assign(np, NONE);
    last.assign(np, 0);
    for (int t = 0; t < P.threads; ++t)
      for (uint32_t p = 0; p < np; ++p) {
        first[p] = std::min(first[p], ft[t][p]);
        last[p] = std::max(last[p], lt[t][p]);
      }
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx0, SWG_ERR_OOM, "out of host memory while planning %llu records", (unsigned long long)n);
  } catch (const std::system_error& e) {
    return swg_set_error(ctx0, SWG_ERR_OOM, "cannot start host threads: %s", e.what());
  }
  const uint32_t np = P.n_pairs;
  for (int d = 0; d < n_ctx; ++d) {  // the largest range every context holds: staging block + scratch
    swg_ctx* ctx = ctxs[d];
    SWG_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t budget = device_budget(ctx, true);
    const uint64_t r = swg_range::largest(swg_range::MAX_RANGE, budget, [&](uint64_t m) {
      return (uint64_t)swg_io_block_bytes(m, rec->n_seq) + swg_arena_estimate(m, rec, cfg, false);
    });
    if (r == 0)
      return swg_set_error(ctx0, SWG_ERR_OOM, "context %d: the ranged filter needs more than the %llu bytes of device memory %s", d,
                           (unsigned long long)budget, ctx->mem_limit ? "the memory limit leaves" : "that are free");
    R = std::min(R, r);
  }
  for (int d = 0; d < n_ctx; ++d) {  // (under a limit, a staging block larger than this call's ranges need would take the arena's share)
    swg_ctx* ctx = ctxs[d];
    if (ctx->mem_limit && ctx->io_block && ctx->io_cap > swg_io_block_bytes(R, rec->n_seq)) {
      SWG_HIP(ctx, hipSetDevice(ctx->device));
      SWG_HIP(ctx, hipStreamSynchronize(ctx->stream));
      SWG_HIP(ctx, hipFree(ctx->io_block));
      ctx->io_block = nullptr;
      ctx->io_cap = 0;
    }
  }
  range_of.resize(np);
  uint32_t badp = 0;
  if (swg_range::pack(np, P.count.data(), first.data(), last.data(), R, &ranges, range_of.data(), &badp) != swg_range::PACK_OK)
    return swg_set_error(ctx0, SWG_ERR_RANGE, "a genome pair has %llu records: 2^31 or more records in one genome pair are not supported",
                         (unsigned long long)P.count[badp]);
  static const bool dbg = getenv("SWG_DEBUG") != nullptr;
  if (dbg) fprintf(stderr, "[swg] ranged host call over %llu records: %zu ranges of at most %llu records over %d context(s)\n",
                   (unsigned long long)n, ranges.size(), (unsigned long long)R, n_ctx);
  std::vector<uint32_t> lo(np, 0xffffffffu), hi(np, 0);
  std::vector<swg_stats> rstats(ranges.size());
  std::vector<int> rc_of(n_ctx, SWG_OK);
  const uint32_t* pair = P.pair.data();
  unsigned hc = std::thread::hardware_concurrency();
  const int per = std::max(1, std::min(8, hc ? (int)(hc / (unsigned)n_ctx) : 1));
  try {
    swg_host::run(n_ctx, [&](int d) {
      swg_ctx* ctx = ctxs[d];
      std::vector<uint64_t> idx;
      std::vector<uint8_t> st_sub;
      std::vector<uint32_t> ch_sub;
      for (size_t k = (size_t)d; k < ranges.size(); k += (size_t)n_ctx) {
        const uint64_t m = ranges[k].count;
        idx.resize(m);
        st_sub.resize(m);
        ch_sub.resize(m);
        // the range's record indices, ascending: counts per slice, then every slice fills its part
        const int T = (int)std::min<uint64_t>((uint64_t)per, n / 65536 + 1);
        std::vector<uint64_t> c(T + 1, 0);
        swg_host::run(T, [&](int t) {
          const uint64_t b = n * (uint64_t)t / T, e = n * (uint64_t)(t + 1) / T;
          uint64_t x = 0;
          for (uint64_t i = b; i < e; ++i) x += range_of[pair[i]] == (uint32_t)k;
          c[t + 1] = x;
        });
        for (int t = 0; t < T; ++t) c[t + 1] += c[t];
        swg_host::run(T, [&](int t) {
          const uint64_t b = n * (uint64_t)t / T, e = n * (uint64_t)(t + 1) / T;
          uint64_t w = c[t];
          for (uint64_t i = b; i < e; ++i)
            if (range_of[pair[i]] == (uint32_t)k) idx[w++] = i;
        });
        int rc = swg_filter_gathered(ctx, rec, idx.data(), m, cfg, st_sub.data(), ch_sub.data(), &rstats[k], per);
        if (rc == SWG_ERR_OOM && ranges[k].oversize) {
          const std::string msg = swg_last_error(ctx);
          rc = swg_set_error(ctx, SWG_ERR_OOM, "a genome pair of %llu records does not fit %s (%s)",
                             (unsigned long long)m, what_bounds(ctx).c_str(), msg.c_str());
        }
        if (rc != SWG_OK) {
          rc_of[d] = rc;
          return;
        }
        // results into the caller's arrays; the range's pairs are its own, so their chain bounds are too
        for (uint64_t j = 0; j < m; ++j) {
          const uint64_t i = idx[j];
          status_out[i] = st_sub[j];
          const uint32_t ch = ch_sub[j];
          chain_out[i] = ch;
          if (ch) {
            const uint32_t p = pair[i];
            lo[p] = std::min(lo[p], ch);
            hi[p] = std::max(hi[p], ch);
          }
        }
      }
    });
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx0, SWG_ERR_OOM, "out of host memory in the ranged filter");
  }
  for (int d = 0; d < n_ctx; ++d)
    if (rc_of[d] != SWG_OK) {
      if (d == 0) return rc_of[0];
      const std::string msg = swg_last_error(ctxs[d]);
      return swg_set_error(ctx0, rc_of[d], "context %d of %d: %s", d, n_ctx, msg.c_str());
    }
  if (cfg->scaffold_gap != 0) {
    std::vector<int64_t> shift(np);
    uint64_t total = 0;
    if (!swg_range::shifts(np, lo.data(), hi.data(), P.first.data(), shift.data(), &total))
      return swg_set_error(ctx0, SWG_ERR_RANGE, "%llu kept chains: chain numbers of 2^32 or more are not supported", (unsigned long long)total);
    try {
      swg_host::run(P.threads, [&](int t) {
        const uint64_t b = n * (uint64_t)t / P.threads, e = n * (uint64_t)(t + 1) / P.threads;
        for (uint64_t i = b; i < e; ++i)
          if (chain_out[i]) chain_out[i] = (uint32_t)((int64_t)chain_out[i] + shift[pair[i]]);
      });
    } catch (const std::bad_alloc&) {
      return swg_set_error(ctx0, SWG_ERR_OOM, "out of host memory while renumbering");
    }
  }
  if (stats) {
    *stats = swg_stats{};
    stats->n_in = n;
    for (const swg_stats& a : rstats) {
      add_stats(stats, a);
      stats->device_ms += a.device_ms;
      stats->h2d_ms += a.h2d_ms;
      stats->d2h_ms += a.d2h_ms;
    }
  }
  return SWG_OK;
}
