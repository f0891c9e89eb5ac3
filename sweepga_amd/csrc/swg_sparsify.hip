// Tree sparsification (--sparsify tree:/knn:, src/tree_filter.rs) as an operation on RECORDS: a keep flag per record computed on
// the device, and a filter entry that runs on the kept subset and answers in the caller's record indices.
//
//   sparsify_pairsum   per unordered pair of DIFFERENT genomes (key = smaller id * G + larger id) sum(matches), sum(block_len)
//                      and the record count, u64: runs of one pair along a wavefront summed towards the run's first lane, a small
//                      LDS table per work-group, one atomic per (work-group, pair, quantity), dense G x G table up to 2^20 entries,
//                      open addressing beyond: the scheme of swg_pair_table.h.
//   sparsify_collect   the pairs that occur as a list.  The host turns it into (pair sums, prefixes) and runs THE selection
//                      (swg_tree_select, host/tree_filter.cpp): the strings decide the canonical order of a pair, the tie order and
//                      the hash, the device never sees one.
//   sparsify_mark      one lane per record: genome pair -> bit of the selected-pair bitmap (dense) or probe of the selected-pair
//                      set (built on the host with the same hash) -> keep[i]; equal genomes are never kept (:183-186).
//   compaction         kept_index = swg_flags_count / swg_flags_compact (per-lane popcounts, wavefront + work-group scan, tile
//                      offsets from the project's scan: ascending, so the order of the records is preserved exactly);
//                      sparsify_gather copies the columns the caller gave.
//   sparsify_scatter   status_full[kept_index[j]] = status[j], likewise chain, over zero-filled outputs: every entry is written.
// Integer atomics only.  Sequence ids keep the numbering of the full input: DESIGN section 12 has the evidence that no answer of
// the filter depends on the order of ids.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <thread>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "host/host_internal.h"
#include "host/threads.h"

namespace {

using namespace swg_pair_table;  // the genome-pair table, the run and wavefront helpers, the host entry helpers

enum { D_LISTED = 0, D_BAD, D_KEPT, D_TOTAL };

using SumTable = PairTable<3, false>;  // sums, and the entries of the one list: matches, block length, records
using SumList = PairList<3, false>;

__global__ __launch_bounds__(TB) void sparsify_pairsum_kernel(uint64_t n, uint64_t per_group, const uint32_t* __restrict__ q_id,
                                                              const uint32_t* __restrict__ t_id, const uint32_t* __restrict__ matches,
                                                              const uint32_t* __restrict__ block_len, const uint32_t* __restrict__ seq_genome,
                                                              uint32_t n_seq, uint32_t n_genome, SumTable T,
                                                              unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<3, false> l_pairs;
  __shared__ uint32_t l_bad;
  l_pairs.clear();
  if (threadIdx.x == 0) l_bad = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint64_t b0 = (uint64_t)blockIdx.x * per_group;
  const uint64_t b1 = b0 + per_group < n ? b0 + per_group : n;
  bool bad = false;
  const uint64_t iters = b1 > b0 ? (b1 - b0 + TB - 1) / TB : 0;  // uniform over the work-group
  for (uint64_t it = 0; it < iters; ++it) {
    const uint64_t i = b0 + it * TB + threadIdx.x;
    unsigned long long key = EMPTY;
    unsigned long long v[3] = {0, 0, 0};
    if (i < b1) {
      const uint32_t q = q_id[i], t = t_id[i];
      const uint32_t gq = q < n_seq ? seq_genome[q] : NONE32, gt = t < n_seq ? seq_genome[t] : NONE32;
      if (gq >= n_genome || gt >= n_genome) {
        bad = true;
      } else if (gq != gt) {
        key = (unsigned long long)(gq < gt ? gq : gt) * n_genome + (gq < gt ? gt : gq);
        v[0] = matches[i];
        v[1] = block_len[i];
        v[2] = 1;
      }
    }
    const unsigned long long before = __shfl_up(key, 1);
    const bool head = lane == 0 || key != before;
    const uint64_t heads = __ballot(head);
    if (__ballot(key != EMPTY) == 0) continue;  // wavefront-uniform
    run_sum(v, lane, run_end(heads, lane));
    if (head && key != EMPTY) {
      if (!l_pairs.add(key, v)) table_add<3, false>(T, key, v, 0);  // more pairs in this share than the LDS table takes (shuffled input)
    }
  }
  if (bad) l_bad = 1;
  __syncthreads();
  l_pairs.flush(T, 0);
  if (threadIdx.x == 0 && l_bad) atomicOr(&scalars[D_BAD], 1ull);
}

__global__ __launch_bounds__(TB) void sparsify_collect_kernel(SumTable T, SumList L) { list_slots(T, L); }

// bitmap != nullptr: bit `key` of it; else the open-addressing set (set_keys, set_mask) the host built with hash32
__global__ __launch_bounds__(TB) void sparsify_mark_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                           const uint32_t* __restrict__ seq_genome, uint32_t n_seq, uint32_t n_genome,
                                                           const uint32_t* __restrict__ bitmap, const unsigned long long* __restrict__ set_keys,
                                                           uint32_t set_mask, uint8_t* __restrict__ keep, unsigned long long* __restrict__ scalars) {
  __shared__ unsigned long long l_red[WAVES];
  unsigned long long cnt = 0;
  const uint64_t stride = (uint64_t)gridDim.x * TB;
  for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
    const uint32_t q = q_id[i], t = t_id[i];
    const uint32_t gq = q < n_seq ? seq_genome[q] : NONE32, gt = t < n_seq ? seq_genome[t] : NONE32;
    uint8_t k = 0;
    if (gq < n_genome && gt < n_genome && gq != gt) {
      const unsigned long long key = (unsigned long long)(gq < gt ? gq : gt) * n_genome + (gq < gt ? gt : gq);
      if (bitmap) {
        k = (bitmap[key >> 5] >> (key & 31)) & 1u;
      } else {
        for (uint32_t h = hash32(key) & set_mask;; h = (h + 1) & set_mask) {  // (half the slots are free: the probe ends)
          const unsigned long long s = set_keys[h];
          if (s == key) k = 1;
          if (s == key || s == EMPTY) break;
        }
      }
    }
    keep[i] = k;
    cnt += k;
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) l_red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < WAVES; ++w) s += l_red[w];
    if (s) atomicAdd(&scalars[D_KEPT], s);
  }
}

struct Cols {
  const uint32_t* u32[8];  // q_id, t_id, q_start, q_end, t_start, t_end, matches, block_len (nullptr = absent)
  const double* identity;
  const uint8_t* strand;
};
struct ColsOut {
  uint32_t* u32[8];
  double* identity;
  uint8_t* strand;
};

__global__ __launch_bounds__(TB) void sparsify_gather_kernel(uint64_t m, const uint32_t* __restrict__ kept_index, Cols in, ColsOut out) {
  const uint64_t stride = (uint64_t)gridDim.x * TB;
  for (uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x; j < m; j += stride) {
    const uint32_t i = kept_index[j];
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (in.u32[c]) out.u32[c][j] = in.u32[c][i];
    if (in.identity) out.identity[j] = in.identity[i];
    if (in.strand) out.strand[j] = in.strand[i];
  }
}

__global__ __launch_bounds__(TB) void sparsify_scatter_kernel(uint64_t m, const uint32_t* __restrict__ kept_index, const uint8_t* __restrict__ status,
                                                              const uint32_t* __restrict__ chain, uint8_t* __restrict__ status_full,
                                                              uint32_t* __restrict__ chain_full) {
  const uint64_t stride = (uint64_t)gridDim.x * TB;
  for (uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x; j < m; j += stride) {
    const uint32_t i = kept_index[j];
    status_full[i] = status[j];
    chain_full[i] = chain[j];
  }
}

// ---- the mask --------------------------------------------------------------------------------------------------------------
struct SelCols {
  const uint32_t *q_id, *t_id, *matches, *block_len, *seq_genome;
};

// inside an arena frame; d_keep on the device.  *too_big: a pair's sum reached 2^53 (no selection was made)
int select_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const SelCols& d, const std::vector<std::string>& prefix,
                  uint64_t k_nearest, uint64_t k_farthest, double random_fraction, uint8_t* d_keep, uint64_t* n_kept, bool* too_big) {
  hipStream_t st = ctx->stream;
  *too_big = false;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  const uint64_t all_pairs = (uint64_t)G * (G - 1) / 2;
  const uint64_t pairs_max = std::max<uint64_t>(1, std::min(all_pairs, n));
  SumTable T;
  SumList L;
  SWG_TRY(table_create(ctx, G, pairs_max, false, false, scalars + D_LISTED, &T, &L));
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  const Share share = share_for(ctx, n);
  SWG_LAUNCH(ctx, "sparsify_pairsum", sparsify_pairsum_kernel<<<share.grid, TB, 0, st>>>(n, share.per_group, d.q_id, d.t_id, d.matches, d.block_len,
                                                                                           d.seq_genome, n_seq, G, T, scalars));
  SWG_KERNEL_CHECK(ctx);
  SWG_LAUNCH(ctx, "sparsify_collect", sparsify_collect_kernel<<<(unsigned)((T.slots + TB - 1) / TB), TB, 0, st>>>(T, L));
  SWG_KERNEL_CHECK(ctx);
  uint64_t h[D_TOTAL];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  if (h[D_BAD]) return swg_set_error(ctx, SWG_ERR_INVALID, "tree select: a sequence id >= n_seq or a genome id >= n_genome");
  std::vector<SumList::Entry> lists[1];
  SWG_TRY(list_fetch(ctx, "tree select", L, h + D_LISTED, lists));
  const std::vector<SumList::Entry>& list = lists[0];
  // the listing order is whatever the atomics made it: the selection does not depend on it (a total order per genome, one hash per pair)
  std::vector<swg_tree_pair> pairs(list.size());
  for (size_t k = 0; k < list.size(); ++k) {
    if (list[k].v[0] >= SWG_TREE_SUM_LIMIT || list[k].v[1] >= SWG_TREE_SUM_LIMIT) {
      *too_big = true;
      return SWG_OK;
    }
    uint32_t a = (uint32_t)(list[k].key / G), b = (uint32_t)(list[k].key % G);
    if (prefix[b] < prefix[a]) std::swap(a, b);
    pairs[k] = swg_tree_pair{a, b, (double)list[k].v[0], (double)list[k].v[1]};
  }
  std::vector<uint8_t> selected;
  swg_tree_select(prefix, pairs, k_nearest, k_farthest, random_fraction, &selected);
  // the selected pairs for the device: a bitmap over the dense keys, or an open-addressing set
  std::vector<uint32_t> bits;
  std::vector<unsigned long long> set;
  uint32_t* d_bits = nullptr;
  unsigned long long* d_set = nullptr;
  uint32_t set_mask = 0;
  if (!T.keys) {  // (dense: slots = G x G)
    bits.assign((T.slots + 31) / 32, 0);
    for (size_t k = 0; k < list.size(); ++k)
      if (selected[k]) bits[list[k].key >> 5] |= 1u << (list[k].key & 31);
    d_bits = swg_alloc<uint32_t>(ctx, bits.size());
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemcpyAsync(d_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  } else {
    uint64_t n_sel = 0;
    for (uint8_t s : selected) n_sel += s;
    set.assign(pow2_at_least(2 * n_sel), EMPTY);
    set_mask = (uint32_t)(set.size() - 1);
    for (size_t k = 0; k < list.size(); ++k) {
      if (!selected[k]) continue;
      uint32_t s = hash32(list[k].key) & set_mask;
      while (set[s] != EMPTY) s = (s + 1) & set_mask;
      set[s] = list[k].key;
    }
    d_set = swg_alloc<unsigned long long>(ctx, set.size());
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemcpyAsync(d_set, set.data(), set.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
  }
  SWG_LAUNCH(ctx, "sparsify_mark", sparsify_mark_kernel<<<grid_for(ctx, n), TB, 0, st>>>(n, d.q_id, d.t_id, d.seq_genome, n_seq, G, d_bits, d_set,
                                                                                           set_mask, d_keep, scalars));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + D_KEPT, h, 1));  // (synchronises: bits / set may go now)
  if (n_kept) *n_kept = h[0];
  return SWG_OK;
}

// columns, seq_genome and keep on the host (staged in the arena) or on the device
int select_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome,
               const std::vector<std::string>& prefix, uint64_t k_nearest, uint64_t k_farthest, double random_fraction, uint8_t* keep,
               uint64_t* n_kept, bool* too_big) {
  if (!ctx) return SWG_ERR_INVALID;
  *too_big = false;
  if (n_kept) *n_kept = 0;
  if (!rec) return swg_set_error(ctx, SWG_ERR_INVALID, "tree select: NULL records");
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  if (n == 0) return SWG_OK;
  if (!rec->q_id || !rec->t_id || !rec->matches || !rec->block_len || !seq_genome || !keep)
    return swg_set_error(ctx, SWG_ERR_INVALID, "tree select: NULL column (q_id, t_id, matches, block_len, seq_genome are read, keep is written)");
  if (n_seq == 0 || n_genome == 0 || prefix.size() != n_genome)
    return swg_set_error(ctx, SWG_ERR_INVALID, "tree select: records without sequences or genomes");
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "tree select: 2^31 records or more in one call");
  if (!(random_fraction >= 0.0) && !(random_fraction < 0.0)) return swg_set_error(ctx, SWG_ERR_INVALID, "tree select: random_fraction is NaN");
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SWG_TRY(reserve_first(ctx, (size_t)n * 24 + (size_t(32) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    SelCols d{rec->q_id, rec->t_id, rec->matches, rec->block_len, seq_genome};
    uint8_t* d_keep = keep;
    if (!on_device) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&d.q_id, &d.t_id, &d.matches, &d.block_len}) s.add(col, n);
      s.add(&d.seq_genome, n_seq);
      d_keep = swg_alloc<uint8_t>(ctx, n);  // (a kernel fills it)
      SWG_TRY(s.run());
    }
    SWG_TRY(select_device(ctx, n, n_seq, n_genome, d, prefix, k_nearest, k_farthest, random_fraction, d_keep, n_kept, too_big));
    if (!on_device && !*too_big) {
      SWG_HIP(ctx, hipMemcpyAsync(keep, d_keep, n, hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));
    }
    return SWG_OK;
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome,
                const char* const* genome_prefix, uint64_t k_nearest, uint64_t k_farthest, double random_fraction, uint8_t* keep,
                uint64_t* n_kept) {
  if (!ctx) return SWG_ERR_INVALID;
  try {
    if (n_genome && !genome_prefix) return swg_set_error(ctx, SWG_ERR_INVALID, "tree select: NULL genome_prefix");
    std::vector<std::string> prefix(n_genome);
    for (uint32_t g = 0; g < n_genome; ++g) {
      if (!genome_prefix[g]) return swg_set_error(ctx, SWG_ERR_INVALID, "tree select: genome_prefix[%u] is NULL", g);
      prefix[g] = genome_prefix[g];
    }
    bool too_big = false;
    SWG_TRY(select_run(ctx, rec, on_device, seq_genome, n_genome, prefix, k_nearest, k_farthest, random_fraction, keep, n_kept, &too_big));
    if (too_big)
      return swg_set_error(ctx, SWG_ERR_RANGE, "tree select: a genome pair's sum of matches or block lengths reaches 2^53 (the reference "
                           "accumulates in f64: beyond that the integer sums are other numbers)");
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

// ---- the subset filter -----------------------------------------------------------------------------------------------------
size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

int subset_block_reserve(swg_ctx* ctx, size_t bytes) {
  if (ctx->subset_cap >= bytes) return SWG_OK;
  SWG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->subset_block) {
    SWG_HIP(ctx, hipFree(ctx->subset_block));
    ctx->subset_block = nullptr;
    ctx->subset_cap = 0;
  }
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess)
    return swg_set_error(ctx, SWG_ERR_OOM, "hipMalloc of %zu bytes for the compacted columns failed: %s", bytes, hipGetErrorString(e));
  ctx->subset_block = static_cast<char*>(p);
  ctx->subset_cap = bytes;
  return SWG_OK;
}

int subset_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg, uint8_t* status_full, uint32_t* chain_full,
                  swg_stats* stats) {
  const uint64_t n = rec->n;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "subset filter: 2^31 records or more in one call");
  if (!rec->q_id || !rec->t_id || !status_full || !chain_full) return swg_set_error(ctx, SWG_ERR_INVALID, "subset filter: NULL column");
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SWG_TRY(reserve_first(ctx, size_t(8) << 20));
  const Cols in{{rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end, rec->matches, rec->block_len}, rec->identity, rec->strand};
  uint64_t m = 0;
  uint32_t* kept_index = nullptr;
  uint8_t* status_sub = nullptr;
  uint32_t* chain_sub = nullptr;
  ColsOut out{};
  const uint64_t limit = ctx->mem_limit;
  // compaction: count, size the block that outlives this arena frame, list, gather
  SWG_TRY(swg_run_with_arena(ctx, [&]() -> int {
    unsigned long long* d_total = swg_alloc<unsigned long long>(ctx, 1);
    SWG_CHECK_ARENA(ctx);
    swg_flag_scan fs;
    SWG_TRY(swg_flags_count(ctx, keep, n, &fs, reinterpret_cast<uint64_t*>(d_total)));
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(d_total), &m, 1));
    if (m == 0) return SWG_OK;
    size_t bytes = al256(m * 4) + al256(m) + al256(m * 4);  // kept_index, status, chain
    for (int c = 0; c < 8; ++c)
      if (in.u32[c]) bytes += al256(m * 4);
    if (in.identity) bytes += al256(m * 8);
    if (in.strand) bytes += al256(m);
    if (limit) {
      if (bytes >= limit)
        return swg_set_error(ctx, SWG_ERR_OOM, "subset filter: %zu bytes of compacted columns do not fit the memory limit of %llu bytes", bytes,
                             (unsigned long long)limit);
      if (ctx->subset_cap > bytes) {  // exactly this call's size under a limit
        SWG_HIP(ctx, hipStreamSynchronize(st));
        SWG_HIP(ctx, hipFree(ctx->subset_block));
        ctx->subset_block = nullptr;
        ctx->subset_cap = 0;
      }
    }
    SWG_TRY(subset_block_reserve(ctx, bytes));
    char* p = ctx->subset_block;
    auto take = [&](size_t b) {
      char* q = p;
      p += al256(b);
      return q;
    };
    kept_index = reinterpret_cast<uint32_t*>(take(m * 4));
    status_sub = reinterpret_cast<uint8_t*>(take(m));
    chain_sub = reinterpret_cast<uint32_t*>(take(m * 4));
    for (int c = 0; c < 8; ++c) out.u32[c] = in.u32[c] ? reinterpret_cast<uint32_t*>(take(m * 4)) : nullptr;
    out.identity = in.identity ? reinterpret_cast<double*>(take(m * 8)) : nullptr;
    out.strand = in.strand ? reinterpret_cast<uint8_t*>(take(m)) : nullptr;
    SWG_TRY(swg_flags_compact(ctx, fs, kept_index));
    SWG_LAUNCH(ctx, "sparsify_gather", sparsify_gather_kernel<<<grid_for(ctx, m), TB, 0, st>>>(m, kept_index, in, out));
    SWG_KERNEL_CHECK(ctx);
    return SWG_OK;
  }));
  if (stats) *stats = swg_stats{};
  int rc = SWG_OK;
  if (m) {
    swg_records sub = *rec;
    sub.n = m;
    sub.q_id = out.u32[0];
    sub.t_id = out.u32[1];
    sub.q_start = out.u32[2];
    sub.q_end = out.u32[3];
    sub.t_start = out.u32[4];
    sub.t_end = out.u32[5];
    sub.matches = out.u32[6];
    sub.block_len = out.u32[7];
    sub.identity = out.identity;
    sub.strand = out.strand;
    if (limit) {  // the filter call inside runs under what the limit leaves beside the compacted columns
      ctx->mem_limit = limit - ctx->subset_cap;
      if ((uint64_t)ctx->arena_cap + ctx->io_cap + ctx->range_cap > ctx->mem_limit && ctx->arena) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(ctx->arena);
        ctx->arena = nullptr;
        ctx->arena_cap = 0;
      }
    }
    rc = swg_filter_device(ctx, &sub, cfg, status_sub, chain_sub, stats);
    ctx->mem_limit = limit;
  }
  if (rc == SWG_OK) {
    rc = [&]() -> int {
      SWG_HIP(ctx, hipMemsetAsync(status_full, 0, n, st));
      SWG_HIP(ctx, hipMemsetAsync(chain_full, 0, n * sizeof(uint32_t), st));
      if (m) {
        SWG_LAUNCH(ctx, "sparsify_scatter",
                   sparsify_scatter_kernel<<<grid_for(ctx, m), TB, 0, st>>>(m, kept_index, status_sub, chain_sub, status_full, chain_full));
        SWG_KERNEL_CHECK(ctx);
      }
      return SWG_OK;
    }();
  }
  if (stats) stats->n_in = n;
  if (limit && ctx->subset_block) {  // under a limit the block does not outlive the call
    (void)hipStreamSynchronize(st);
    (void)hipFree(ctx->subset_block);
    ctx->subset_block = nullptr;
    ctx->subset_cap = 0;
  }
  return rc;
}

int host_threads() {
  const unsigned hc = std::thread::hardware_concurrency();
  return (int)std::max(1u, std::min(hc ? hc : 1u, 16u));
}

// host columns: compacted by host threads, filtered by the unchanged swg_filter / swg_filter_multi, scattered back
int subset_host(swg_ctx* const* ctxs, int n_ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg, uint8_t* status_full,
                uint32_t* chain_full, swg_stats* stats) {
  swg_ctx* ctx = ctxs[0];
  auto filter = [&](const swg_records* r, uint8_t* s, uint32_t* c) {
    return n_ctx > 1 ? swg_filter_multi(ctxs, n_ctx, r, cfg, s, c, stats) : swg_filter(ctx, r, cfg, s, c, stats);
  };
  if (!rec) return swg_set_error(ctx, SWG_ERR_INVALID, "subset filter: NULL records");
  if (!keep || rec->n == 0) return filter(rec, status_full, chain_full);
  const uint64_t n = rec->n;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "subset filter: 2^31 records or more in one call");
  if (!status_full || !chain_full) return swg_set_error(ctx, SWG_ERR_INVALID, "subset filter: NULL output");
  const int T = (int)std::min<uint64_t>(host_threads(), (n + 65535) / 65536);
  std::vector<uint64_t> base(T + 1, 0);
  auto lo = [&](int t) { return n / T * t + std::min<uint64_t>(t, n % T); };
  swg_host::run(T, [&](int t) {
    uint64_t c = 0;
    for (uint64_t i = lo(t); i < lo(t + 1); ++i) c += keep[i] != 0;
    base[t + 1] = c;
  });
  for (int t = 0; t < T; ++t) base[t + 1] += base[t];
  const uint64_t m = base[T];
  const uint32_t* src32[8] = {rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end, rec->matches, rec->block_len};
  struct Free {
    void operator()(void* p) const { std::free(p); }
  };
  std::unique_ptr<char, Free> store;
  uint32_t* dst32[8] = {};
  double* dst_id = nullptr;
  uint8_t *dst_strand = nullptr, *status_sub = nullptr;
  uint32_t* chain_sub = nullptr;
  {
    size_t bytes = 0;
    auto room = [&](size_t b) {
      const size_t at = bytes;
      bytes += (b + 63) & ~size_t(63);
      return at;
    };
    size_t at32[8], at_id = 0, at_strand = 0;
    for (int c = 0; c < 8; ++c) at32[c] = src32[c] ? room(m * 4) : 0;
    if (rec->identity) at_id = room(m * 8);
    if (rec->strand) at_strand = room(m);
    const size_t at_status = room(m), at_chain = room(m * 4);
    store.reset(static_cast<char*>(std::malloc(bytes ? bytes : 1)));
    if (!store) return swg_set_error(ctx, SWG_ERR_OOM, "subset filter: out of host memory for %zu bytes of compacted columns", bytes);
    for (int c = 0; c < 8; ++c)
      if (src32[c]) dst32[c] = reinterpret_cast<uint32_t*>(store.get() + at32[c]);
    if (rec->identity) dst_id = reinterpret_cast<double*>(store.get() + at_id);
    if (rec->strand) dst_strand = reinterpret_cast<uint8_t*>(store.get() + at_strand);
    status_sub = reinterpret_cast<uint8_t*>(store.get() + at_status);
    chain_sub = reinterpret_cast<uint32_t*>(store.get() + at_chain);
  }
  swg_host::run(T, [&](int t) {
    uint64_t j = base[t];
    for (uint64_t i = lo(t); i < lo(t + 1); ++i) {
      if (!keep[i]) continue;
      for (int c = 0; c < 8; ++c)
        if (src32[c]) dst32[c][j] = src32[c][i];
      if (dst_id) dst_id[j] = rec->identity[i];
      if (dst_strand) dst_strand[j] = rec->strand[i];
      ++j;
    }
  });
  if (stats) *stats = swg_stats{};
  if (m) {
    swg_records sub = *rec;
    sub.n = m;
    sub.q_id = dst32[0];
    sub.t_id = dst32[1];
    sub.q_start = dst32[2];
    sub.q_end = dst32[3];
    sub.t_start = dst32[4];
    sub.t_end = dst32[5];
    sub.matches = dst32[6];
    sub.block_len = dst32[7];
    sub.identity = dst_id;
    sub.strand = dst_strand;
    SWG_TRY(filter(&sub, status_sub, chain_sub));
  }
  if (stats) stats->n_in = n;
  swg_host::run(T, [&](int t) {
    uint64_t j = base[t];
    for (uint64_t i = lo(t); i < lo(t + 1); ++i) {
      const bool k = keep[i] != 0;
      status_full[i] = k ? status_sub[j] : 0;
      chain_full[i] = k ? chain_sub[j] : 0;
      j += k;
    }
  });
  return SWG_OK;
}

// mask of a handle: the device route, or (PAF handles whose columns are not what the text pass reads, and sums of 2^53 or more)
// the text route's verdicts
int handle_select(swg_ctx* ctx, const swg_tree_handle_view& v, const swg_records& rec, uint64_t k_nearest, uint64_t k_farthest,
                  double random_fraction, uint8_t* keep, uint64_t* n_kept, int* route) {
  const uint64_t n = rec.n;
  if (n_kept) *n_kept = 0;
  if (route) *route = SWG_TREE_ROUTE_DEVICE;
  if (n == 0) return SWG_OK;
  if (!keep) return SWG_ERR_INVALID;
  bool text_route = v.text_route;
  if (!text_route) {
    if (!ctx) return SWG_ERR_INVALID;
    bool too_big = false;
    SWG_TRY(select_run(ctx, &rec, false, rec.seq_genome_two, rec.n_genome_two, *v.prefix_two, k_nearest, k_farthest, random_fraction, keep,
                       n_kept, &too_big));
    if (!too_big) return SWG_OK;
    if (!v.text) return swg_set_error(ctx, SWG_ERR_RANGE, "tree select: a genome pair's sum of matches or lengths reaches 2^53");
    text_route = true;
  }
  if (route) *route = SWG_TREE_ROUTE_TEXT;
  const int rc = swg_tree_text_mask(v.text, v.text_len, k_nearest, k_farthest, random_fraction, v.rec_off, n, keep, n_kept);
  if (rc != SWG_OK && ctx) return swg_set_error(ctx, rc, "tree select: the text route failed");
  return rc;
}

}  // namespace

extern "C" int swg_tree_select_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                       const char* const* genome_prefix, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                                       uint8_t* keep, uint64_t* n_kept) {
  return records_abi(ctx, rec, false, seq_genome, n_genome, genome_prefix, k_nearest, k_farthest, random_fraction, keep, n_kept);
}

extern "C" int swg_tree_select_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                              const char* const* genome_prefix, uint64_t k_nearest, uint64_t k_farthest,
                                              double random_fraction, uint8_t* keep, uint64_t* n_kept) {
  return records_abi(ctx, rec, true, seq_genome, n_genome, genome_prefix, k_nearest, k_farthest, random_fraction, keep, n_kept);
}

extern "C" int swg_filter_subset_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg, uint8_t* status_out,
                                        uint32_t* chain_out, swg_stats* stats) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!keep || !rec || rec->n == 0) return swg_filter_device(ctx, rec, cfg, status_out, chain_out, stats);
  if (!cfg) return swg_set_error(ctx, SWG_ERR_INVALID, "subset filter: NULL config");
  try {
    return subset_device(ctx, rec, keep, cfg, status_out, chain_out, stats);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_filter_subset(swg_ctx* ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg, uint8_t* status_out,
                                 uint32_t* chain_out, swg_stats* stats) {
  if (!ctx) return SWG_ERR_INVALID;
  try {
    return subset_host(&ctx, 1, rec, keep, cfg, status_out, chain_out, stats);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_filter_subset_multi(swg_ctx* const* ctxs, int n_ctx, const swg_records* rec, const uint8_t* keep, const swg_config* cfg,
                                       uint8_t* status_out, uint32_t* chain_out, swg_stats* stats) {
  if (!ctxs || n_ctx < 1 || !ctxs[0]) return SWG_ERR_INVALID;
  try {
    return subset_host(ctxs, n_ctx, rec, keep, cfg, status_out, chain_out, stats);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctxs[0], SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_paf_tree_select(swg_ctx* ctx, const swg_paf* p, uint64_t k_nearest, uint64_t k_farthest, double random_fraction, int threads,
                                   uint8_t* keep, uint64_t* n_kept, int* route) {
  (void)threads;  // (the text route is one pass on one thread, the device route has no host part worth threads)
  if (!p) return SWG_ERR_INVALID;
  try {
    swg_tree_handle_view v;
    swg_paf_tree_view(p, &v);
    return handle_select(ctx, v, *v.rec, k_nearest, k_farthest, random_fraction, keep, n_kept, route);
  } catch (const std::bad_alloc&) {
    return ctx ? swg_set_error(ctx, SWG_ERR_OOM, "out of host memory") : SWG_ERR_OOM;
  }
}

// apply_tree_filter_to_1aln (src/tree_filter.rs:286-…) sums aln.matches over aln.query_end - aln.query_start (:314-317), not over
// the record's block length (query span + target span, src/unified_filter.rs:107-112): the length column is rebuilt here.
extern "C" int swg_aln_tree_select(swg_ctx* ctx, const swg_aln* a, uint64_t k_nearest, uint64_t k_farthest, double random_fraction,
                                   uint8_t* keep, uint64_t* n_kept) {
  if (!a) return SWG_ERR_INVALID;
  try {
    swg_tree_handle_view v;
    swg_aln_tree_view(a, &v);
    swg_records rec = *v.rec;
    std::vector<uint32_t> span(rec.n);
    for (uint64_t i = 0; i < rec.n; ++i) span[i] = rec.q_end[i] - rec.q_start[i];
    rec.block_len = span.data();
    return handle_select(ctx, v, rec, k_nearest, k_farthest, random_fraction, keep, n_kept, nullptr);
  } catch (const std::bad_alloc&) {
    return ctx ? swg_set_error(ctx, SWG_ERR_OOM, "out of host memory") : SWG_ERR_OOM;
  }
}
