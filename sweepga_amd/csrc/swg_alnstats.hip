// alnstats (src/bin/alnstats.rs:103-161) over record columns on the device: the integer results of parse_paf for ALL records
// and, from the same launches, for the records a filter call KEPT (status != 0).  Everything is a sum, a count, a minimum or a
// maximum of integers keyed by something the host supplies, so the results do not depend on the order of the work:
//
//   alnstats_seqpair   distinct (q_id, t_id): open-addressing hash SET over q_id * n_seq + t_id (bit 63 of a slot: some KEPT
//                      record has the pair).  Runs of one pair inside a wavefront insert once.
//   alnstats_reduce    the scalar sums and counts (registers -> wavefront -> work-group -> one atomic per work-group and
//                      quantity); per ordered genome pair sum(bases), sum(matches) and min(record) -- runs of one pair are
//                      summed across the lanes of the wavefront first (segmented add under a ballot of "same key as the lane
//                      before"), then in a small LDS table of the work-group, then one atomic per (work-group, pair, quantity);
//                      per sequence max(2 * record + side), the line that has the last word on its length.  A work-group walks
//                      its contiguous share of the records BACKWARDS: the first value it offers a sequence is its largest, every
//                      later one is turned away by a plain load.
//   alnstats_collect   the occupied entries of the genome-pair table as a list (the host orders it by first record).
//
// The genome-pair table is keyed by gq * G + gt under ANY sequence -> genome map (a parameter: alnstats' last-'#' rule here,
// the filter's two-part prefix for the tree sparsification): dense G x G while that is small, open addressing over the pairs
// that occur beyond it -- at most the distinct (q_id, t_id) pairs, which the first kernel has counted by then.  The table, its
// LDS staging and its listing are swg_pair_table.h's, shared with swg_sparsify.hip and swg_breadth.hip.
// Integer atomics only; no floating point.
#include <algorithm>
#include <new>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;  // the genome-pair table, the run and wavefront helpers, the host entry helpers
constexpr unsigned long long KEPT_BIT = 1ull << 63;
enum { S_MAPPINGS = 0, S_BASES, S_MATCHES, S_SELF, S_INTER_GENOME, S_INTER_CHR, S_COUNT };
// device scalars: [set][S_COUNT], then distinct pairs [2], listed genome pairs [2], bad-id flag
enum { D_DISTINCT = 2 * S_COUNT, D_LISTED = D_DISTINCT + 2, D_BAD = D_LISTED + 2, D_TOTAL };

using StatTable = PairTable<4, true>;  // sums: bases ALL, matches ALL, bases KEPT, matches KEPT
using StatList = PairList<4, true>;    // entries: bases, matches, first record of the set

// ---- distinct (q_id, t_id) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void alnstats_seqpair_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                              const uint8_t* __restrict__ status, uint32_t n_seq,
                                                              unsigned long long* __restrict__ keys, uint32_t mask,
                                                              unsigned long long* __restrict__ scalars) {
  const int lane = threadIdx.x & 63;
  uint32_t new_all = 0, new_kept = 0;
  const uint64_t stride = (uint64_t)gridDim.x * TB;
  for (uint64_t base = (uint64_t)blockIdx.x * TB; base < n; base += stride) {  // uniform trip count per work-group
    const uint64_t i = base + threadIdx.x;
    unsigned long long key = EMPTY;
    bool kept = false;
    if (i < n) {
      const uint32_t q = q_id[i], t = t_id[i];
      if (q < n_seq && t < n_seq) {  // (ids out of range are reported by the reduction kernel)
        key = (unsigned long long)q * n_seq + t;
        kept = status && status[i] != 0;
      }
    }
    const unsigned long long before = __shfl_up(key, 1);
    const bool head = lane == 0 || key != before;
    const uint64_t heads = __ballot(head), keptmask = __ballot(kept);
    if (head && key != EMPTY) {
      const bool any_kept = (keptmask & lane_range(lane, run_end(heads, lane))) != 0;
      uint32_t h = hash32(key) & mask;
      for (;;) {
        unsigned long long k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == EMPTY) {
          k = atomicCAS(&keys[h], EMPTY, key);
          if (k == EMPTY) {
            k = key;
            ++new_all;
          }
        }
        if ((k & ~KEPT_BIT) == key) {
          if (any_kept && !(k & KEPT_BIT) && !(atomicOr(&keys[h], KEPT_BIT) & KEPT_BIT)) ++new_kept;
          break;
        }
        h = (h + 1) & mask;
      }
    }
  }
  const unsigned long long a = wave_sum(new_all), k = wave_sum(new_kept);
  if (lane == 0) {
    if (a) atomicAdd(&scalars[D_DISTINCT], a);
    if (k) atomicAdd(&scalars[D_DISTINCT + 1], k);
  }
}

// ---- sums, genome-pair table, last line per sequence ----------------------------------------------------------------------
__device__ __forceinline__ void offer_last(uint32_t* slot, uint32_t v) {
  if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(slot, v);
}

__global__ __launch_bounds__(TB) void alnstats_reduce_kernel(uint64_t n, uint64_t per_group, const uint32_t* __restrict__ q_id,
                                                             const uint32_t* __restrict__ t_id, const uint32_t* __restrict__ q_start,
                                                             const uint32_t* __restrict__ q_end, const uint32_t* __restrict__ matches,
                                                             const uint8_t* __restrict__ status, const uint32_t* __restrict__ seq_genome,
                                                             uint32_t n_seq, uint32_t n_genome, StatTable T,
                                                             uint32_t* __restrict__ seq_last,  // [2][n_seq]: 2 * record + side + 1, 0 = none
                                                             unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<4, true> l_pairs;
  __shared__ unsigned long long l_red[WAVES][2 * S_COUNT];
  __shared__ uint32_t l_bad;
  l_pairs.clear();
  if (threadIdx.x == 0) l_bad = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * per_group;
  const uint64_t b1 = b0 + per_group < n ? b0 + per_group : n;
  unsigned long long acc[2][S_COUNT] = {};
  bool bad = false;
  const uint64_t iters = b1 > b0 ? (b1 - b0 + TB - 1) / TB : 0;
  for (uint64_t it = iters; it-- > 0;) {  // backwards: see the head of the file
    const uint64_t i = b0 + it * TB + threadIdx.x;
    unsigned long long key = EMPTY;
    unsigned long long v[4] = {0, 0, 0, 0};
    bool kept = false;
    if (i < b1) {
      const uint32_t q = q_id[i], t = t_id[i];
      const uint32_t gq = q < n_seq ? seq_genome[q] : NONE32, gt = t < n_seq ? seq_genome[t] : NONE32;
      if (gq >= n_genome || gt >= n_genome) {
        bad = true;
      } else {
        const uint32_t len = q_end[i] - q_start[i], m = matches[i];
        kept = status && status[i] != 0;
        const int cls = q == t ? S_SELF : gq != gt ? S_INTER_GENOME : S_INTER_CHR;  // the precedence of :140-152
        const uint32_t vq = 2u * (uint32_t)i + 1u, vt = vq + 1u;
        acc[0][S_MAPPINGS] += 1;
        acc[0][S_BASES] += len;
        acc[0][S_MATCHES] += m;
        acc[0][S_SELF] += cls == S_SELF;  // (no indexing by cls: the counters stay in registers)
        acc[0][S_INTER_GENOME] += cls == S_INTER_GENOME;
        acc[0][S_INTER_CHR] += cls == S_INTER_CHR;
        offer_last(&seq_last[q], vq);
        offer_last(&seq_last[t], vt);
        if (kept) {
          acc[1][S_MAPPINGS] += 1;
          acc[1][S_BASES] += len;
          acc[1][S_MATCHES] += m;
          acc[1][S_SELF] += cls == S_SELF;
          acc[1][S_INTER_GENOME] += cls == S_INTER_GENOME;
          acc[1][S_INTER_CHR] += cls == S_INTER_CHR;
          offer_last(&seq_last[(size_t)n_seq + q], vq);
          offer_last(&seq_last[(size_t)n_seq + t], vt);
        }
        if (cls == S_INTER_GENOME) {
          key = (unsigned long long)gq * n_genome + gt;
          v[0] = len;
          v[1] = m;
          v[2] = kept ? len : 0;
          v[3] = kept ? m : 0;
        }
      }
    }
    // runs of one genome pair along the lanes: summed towards the run's first lane
    const unsigned long long before = __shfl_up(key, 1);
    const bool head = lane == 0 || key != before;
    const uint64_t heads = __ballot(head), keptmask = __ballot(kept);
    if (__ballot(key != EMPTY) == 0) continue;  // wavefront-uniform
    const int end = run_end(heads, lane);
    run_sum(v, lane, end);
    if (head && key != EMPTY) {
      const uint64_t kf = keptmask & lane_range(lane, end);
      const uint32_t f_all = (uint32_t)i, f_kept = kf ? (uint32_t)(i - lane + __builtin_ctzll(kf)) : NONE32;
      if (!l_pairs.add(key, v, f_all, f_kept))
        table_add<4, true>(T, key, v, 0, f_all, f_kept);  // more pairs in this share than the LDS table takes (shuffled input)
    }
  }
  if (bad) l_bad = 1;
  __syncthreads();
  l_pairs.flush(T, 0);
#pragma unroll
  for (int k = 0; k < 2 * S_COUNT; ++k) {
    const unsigned long long s = wave_sum(acc[k / S_COUNT][k % S_COUNT]);
    if (lane == 0) l_red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 2 * S_COUNT) {
    unsigned long long s = 0;
    for (int w = 0; w < WAVES; ++w) s += l_red[w][threadIdx.x];
    if (s) atomicAdd(&scalars[threadIdx.x], s);
  }
  if (threadIdx.x == 0 && l_bad) atomicOr(&scalars[D_BAD], 1ull);
}

// ---- the occupied genome pairs as lists ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void alnstats_collect_kernel(StatTable T, StatList L) { list_slots(T, L); }

struct DevCols {
  const uint32_t *q_id, *t_id, *q_start, *q_end, *matches, *seq_genome;
  const uint8_t* status;
};

// inside an arena frame
int alnstats_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const DevCols& d, swg_alnstats_result* all,
                    swg_alnstats_result* kept) {
  hipStream_t st = ctx->stream;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  uint32_t* seq_last = swg_alloc<uint32_t>(ctx, 2 * (size_t)n_seq);
  // distinct (q_id, t_id): at most min(n, n_seq^2) keys in twice the slots
  const uint64_t seq_pairs_max = (uint64_t)n_seq * n_seq < n ? (uint64_t)n_seq * n_seq : n;
  const uint64_t set_cap = pow2_at_least(2 * seq_pairs_max);
  unsigned long long* set_keys = swg_alloc<unsigned long long>(ctx, set_cap);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  SWG_HIP(ctx, hipMemsetAsync(seq_last, 0, 2 * (size_t)n_seq * sizeof(uint32_t), st));
  SWG_HIP(ctx, hipMemsetAsync(set_keys, 0xff, set_cap * sizeof(unsigned long long), st));
  SWG_LAUNCH(ctx, "alnstats_seqpair", alnstats_seqpair_kernel<<<grid_for(ctx, n), TB, 0, st>>>(n, d.q_id, d.t_id, d.status, n_seq, set_keys,
                                                                                                 (uint32_t)(set_cap - 1), scalars));
  SWG_KERNEL_CHECK(ctx);
  uint64_t distinct[2];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + D_DISTINCT, distinct, 2));
  // genome pairs that occur <= distinct sequence pairs
  const uint64_t g2 = (uint64_t)G * G;
  const uint64_t pairs_max = g2 < distinct[0] ? g2 : distinct[0];
  StatTable T;
  StatList L;
  SWG_TRY(table_create(ctx, G, pairs_max, false, d.status != nullptr, scalars + D_LISTED, &T, &L));
  const Share share = share_for(ctx, n);
  SWG_LAUNCH(ctx, "alnstats_reduce", alnstats_reduce_kernel<<<share.grid, TB, 0, st>>>(n, share.per_group, d.q_id, d.t_id, d.q_start, d.q_end,
                                                                                         d.matches, d.status, d.seq_genome, n_seq, G, T, seq_last,
                                                                                         scalars));
  SWG_KERNEL_CHECK(ctx);
  SWG_LAUNCH(ctx, "alnstats_collect", alnstats_collect_kernel<<<(unsigned)((T.slots + TB - 1) / TB), TB, 0, st>>>(T, L));
  SWG_KERNEL_CHECK(ctx);
  uint64_t h[D_TOTAL];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  if (h[D_BAD]) return swg_set_error(ctx, SWG_ERR_INVALID, "alnstats: a sequence id >= n_seq or a genome id >= n_genome");
  std::vector<StatList::Entry> list[2];
  SWG_TRY(list_fetch(ctx, "alnstats", L, h + D_LISTED, list));
  std::vector<uint32_t> last((size_t)2 * n_seq);
  SWG_HIP(ctx, hipMemcpyAsync(last.data(), seq_last, last.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SWG_HIP(ctx, hipStreamSynchronize(st));
  swg_alnstats_result* res[2] = {all, d.status ? kept : nullptr};
  for (int s = 0; s < 2; ++s) {
    swg_alnstats_result* r = res[s];
    if (!r) continue;
    const uint64_t* c = h + s * S_COUNT;
    r->total_mappings = c[S_MAPPINGS];
    r->total_bases = c[S_BASES];
    r->total_matches = c[S_MATCHES];
    r->self_mappings = c[S_SELF];
    r->inter_genome = c[S_INTER_GENOME];
    r->inter_chromosomal = c[S_INTER_CHR];
    r->chr_pair_count = distinct[s];
    r->pairs.resize(list[s].size());
    for (size_t k = 0; k < list[s].size(); ++k) {
      const StatList::Entry& o = list[s][k];
      r->pairs[k] = swg_alnstats_pair_counts{(uint32_t)(o.key / G), (uint32_t)(o.key % G), o.v[0], o.v[1], o.first};
    }
    r->seq_last.resize(n_seq);
    for (uint32_t q = 0; q < n_seq; ++q) {
      const uint32_t v = last[(size_t)s * n_seq + q];
      r->seq_last[q] = v ? (uint64_t)v - 1 : UINT64_MAX;
    }
  }
  return SWG_OK;
}

void clear_result(swg_alnstats_result* r, uint32_t n_seq) {
  if (!r) return;
  *r = swg_alnstats_result{};
  r->seq_last.assign(n_seq, UINT64_MAX);
}

void hand_over(const swg_alnstats_result& r, swg_alnstats_counts* c) {
  if (!c) return;
  c->total_mappings = r.total_mappings;
  c->total_bases = r.total_bases;
  c->total_matches = r.total_matches;
  c->self_mappings = r.self_mappings;
  c->inter_chromosomal = r.inter_chromosomal;
  c->inter_genome = r.inter_genome;
  c->chr_pair_count = r.chr_pair_count;
  c->n_pairs = r.pairs.size();
  if (c->pairs && c->n_pairs <= c->pair_capacity) std::copy(r.pairs.begin(), r.pairs.end(), c->pairs);
  if (c->seq_last) std::copy(r.seq_last.begin(), r.seq_last.end(), c->seq_last);
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                swg_alnstats_counts* all, swg_alnstats_counts* kept) {
  if (!ctx) return SWG_ERR_INVALID;
  try {
    swg_alnstats_result ra, rk;
    SWG_TRY(swg_alnstats_run(ctx, rec, on_device, seq_genome, n_genome, status, all ? &ra : nullptr, kept && status ? &rk : nullptr));
    hand_over(ra, all);
    if (status) hand_over(rk, kept);
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

int swg_alnstats_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome,
                     const uint8_t* status, swg_alnstats_result* all, swg_alnstats_result* kept) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec) return swg_set_error(ctx, SWG_ERR_INVALID, "alnstats: NULL records");
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  clear_result(all, n_seq);
  clear_result(kept, n_seq);
  if (n == 0) return SWG_OK;
  if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->matches || !seq_genome)
    return swg_set_error(ctx, SWG_ERR_INVALID, "alnstats: NULL column (q_id, t_id, q_start, q_end, matches and seq_genome are read)");
  if (n_seq == 0 || n_genome == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "alnstats: records without sequences or genomes");
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "alnstats: 2^31 records or more in one call");
  if (n_seq > (uint32_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "alnstats: more than 2^31 sequences");
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 64 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    DevCols d{rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->matches, seq_genome, status};
    if (!on_device) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&d.q_id, &d.t_id, &d.q_start, &d.q_end, &d.matches}) s.add(col, n);
      s.add(&d.seq_genome, n_seq);
      s.add(&d.status, n);
      SWG_TRY(s.run());
    }
    return alnstats_device(ctx, n, n_seq, n_genome, d, all, kept);
  });
}

extern "C" int swg_alnstats_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                    const uint8_t* status, swg_alnstats_counts* all, swg_alnstats_counts* kept) {
  return records_abi(ctx, rec, false, seq_genome, n_genome, status, all, kept);
}

extern "C" int swg_alnstats_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                           const uint8_t* status, swg_alnstats_counts* all, swg_alnstats_counts* kept) {
  return records_abi(ctx, rec, true, seq_genome, n_genome, status, all, kept);
}

// Statistics of an open PAF: records and genome map from the handle, the integers from the device, the sequence sizes and the
// handles from the handle's text (host/paf_io.cpp).  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_alnstats(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, swg_alnstats** all_out, swg_alnstats** kept_out) {
  if (all_out) *all_out = nullptr;
  if (kept_out) *kept_out = nullptr;
  if (!p) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_alnstats: NULL handle");
  const uint64_t n = swg_paf_records(p)->n;
  if (n && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_alnstats: NULL context");
  try {
    swg_records rec;
    std::vector<uint32_t> col10;
    const uint32_t* seq_genome = nullptr;
    SWG_TRY(swg_paf_stats_prepare(p, &rec, &col10, &seq_genome));
    swg_alnstats_result res[2];
    if (n) {
      const int rc = swg_alnstats_run(ctx, &rec, false, seq_genome, rec.n_genome_last, status, &res[0], status ? &res[1] : nullptr);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    }
    swg_alnstats** const outs[2] = {all_out, status ? kept_out : nullptr};
    return swg_paf_stats_finish(p, res, outs);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
