// Transitive lift: the closure of every region under the lift of section 23, hop by hop.  The per-axis index
// of swg_lift.hip is built once (swg_lift_index.h); every hop joins its frontier against it and turns the projections P_h and the
// visited set V_{h-1} into the next frontier F_h = P_h \ V_{h-1} and V_h = V_{h-1} u P_h with the library's sorts, scans and flag
// compaction.  A piece is a swg_lift_region whose `reserved` word holds its owner, the caller's region: the pieces of all regions
// are one stream of "regions with an owner", and the ranges, the scan and the tile heads of the lift take them as they are.  Per hop:
//
//   closure_ranges       one thread per frontier slot: the candidate range of a walked piece (lift_candidates), width 0 for a slot
//                        beyond the frontier or a piece shorter than min_len (hop >= 2)
//   (scan)               swg_inclusive_sum_scan_u64 over the widths, per axis: the candidate stream
//   closure_count        tiles of T = 1024 candidates, heads through LDS (lift_tile_heads); a fixed grid, every work-group takes a
//                        contiguous share of the tiles, because the host has not read the stream's length; a candidate counts when it
//                        is a hit of the set with a non-empty other side; one count per work-group and axis
//   (scan)               swg_inclusive_sum_scan_u64 over the 2 G work-group counts: both axes write one projection stream
//   closure_totals       frontier, visited, candidate and projection totals into the scalars -- THE read-back of the hop
//   closure_project      the same tiles again: ranks from wavefront ballots, one 16-byte store {owner << sb | dst_seq, start, end}
//   closure_events       two boundary events per interval of P_h and of V_{h-1}: key (owner, seq), position << 2 | kind with
//                        kind = V start, P start, P end, V end in this order (see closure_edges for why)
//   (sort)               (owner, seq, position) does not fit 64 bits in general: two stable swg_radix_sort_pairs, by position and
//                        kind (34 bits), then by the key gathered through the first permutation (bits(m) + bits(n_seq))
//   closure_deltas       per sorted event +-1 in the low half (P) or the high half (V) of a 64-bit word, and its position
//   (scan)               swg_inclusive_sum_scan_u64: both depths at once.  Every interval closes on its own key, so the running
//                        sums are zero where the key changes and no segmented scan is needed; neither half ever goes below zero
//   closure_edges        flags an event where "in F" (depth_P > 0 and depth_V == 0) or "in V" (depth_P + depth_V > 0) changes
//   (compact)            swg_flags_count / swg_flags_compact per flag column: edges 2 k and 2 k + 1 are piece k
//   closure_pieces       the pieces of F_h and V_h from the edge lists, their numbers into the scalars
//
// and at the end closure_rows (every F_h with its hop into one array and its two sort keys), the same two-pass sort by (region, seq,
// start), and closure_finish (the rows in order, the summaries from runs of one region along the lanes).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "swg_internal.h"
#include "swg_lift_index.h"
#include "swg_pair_table.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;
using namespace swg_lift_ix;
// device scalars after lift_limits': pieces of the frontier and of the visited set, candidates per axis, projections, edges of F and V
enum { D_NF = 3, D_NV = 4, D_CAND = 5, D_PROJ = 7, D_EDGES = 8, D_TOTAL = 10 };
constexpr uint64_t V_ONE = uint64_t(1) << 32;  // the visited depth's unit in the packed depths

struct ClosureProj {
  uint64_t key;  // owner << sb | seq
  uint32_t start, end;
};
static_assert(sizeof(ClosureProj) == 16 && sizeof(swg_closure_row) == 24 && sizeof(swg_closure_summary) == 24 && sizeof(swg_closure_request) == 80,
              "the ABI's sizes");

// hop 0: which regions are pieces (known, not empty), and the regions' own faults
__global__ __launch_bounds__(TB) void closure_seed_kernel(uint64_t m, const swg_lift_region* __restrict__ regions, uint32_t n_seq,
                                                          uint8_t* __restrict__ flags, unsigned long long* __restrict__ scalars) {
  const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (r >= m) return;
  const swg_lift_region g = regions[r];
  unsigned long long bad = 0;
  if (g.reserved != 0) bad |= 2ull;
  if (g.start > g.end) bad |= 4ull;
  if (g.seq >= n_seq && g.seq != UNKNOWN_SEQ) bad |= 8ull;
  if (bad) atomicOr(&scalars[D_BAD], bad);
  flags[r] = !bad && g.seq != UNKNOWN_SEQ && g.start < g.end;
}

__global__ __launch_bounds__(TB) void closure_seed_pieces_kernel(uint64_t m, const uint32_t* __restrict__ list, const swg_lift_region* __restrict__ regions,
                                                                 swg_lift_region* __restrict__ out, unsigned long long* __restrict__ scalars) {
  const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const uint64_t total = scalars[D_NF];
  if (k == 0) scalars[D_NV] = total;
  if (k >= total || k >= m) return;
  const uint32_t r = list[k];
  swg_lift_region g = regions[r];
  g.reserved = r;
  out[k] = g;
}

__global__ __launch_bounds__(TB) void closure_ranges_kernel(uint64_t cap, const swg_lift_region* __restrict__ F, const unsigned long long* __restrict__ scalars,
                                                            uint32_t hop, uint32_t min_len, uint64_t n, const uint64_t* __restrict__ keys,
                                                            const uint64_t* __restrict__ M, int pb, uint64_t max_start, uint64_t* __restrict__ w,
                                                            uint32_t* __restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= cap) return;
  uint64_t width = 0;
  uint32_t p0 = 0;
  if (i < scalars[D_NF]) {
    const swg_lift_region g = F[i];
    if (hop == 1 || g.end - g.start >= min_len) width = lift_candidates(n, keys, M, pb, max_start, g.seq, g.start, g.end, &p0);
  }
  w[i] = width;
  first[i] = p0;
}

struct ClosureJoin {
  uint64_t cap;            // frontier slots (the pieces come first; the rest have no candidates)
  const swg_lift_region* F;
  const uint64_t* W;       // [cap] inclusive scan of the widths
  const uint32_t* first;   // [cap] p0
  const uint32_t *V, *E;   // the index: values and ends in sorted order
  uint32_t axis, set;
  int sb;                  // bits of a sequence id in a projection's key
  LiftCols c;
  uint64_t* block;         // [2][gridDim.x]: count pass: the projections of (axis, work-group); write pass: their inclusive scan
  ClosureProj* proj;
  uint64_t n_proj;
};

template <bool WRITE>
__device__ __forceinline__ void closure_tiles(const ClosureJoin& J) {
  __shared__ uint32_t l_hs[T];  // lift_tile_heads' four
  __shared__ uint32_t l_hreg[T];
  __shared__ uint32_t l_ha[T];
  __shared__ uint32_t l_hbase[T];
  __shared__ uint32_t l_wave[ITEMS][WAVES];
  __shared__ uint64_t l_span[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t C = J.W[J.cap - 1], ntiles = (C + T - 1) / T, share = (ntiles + gridDim.x - 1) / gridDim.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * share, t1 = t0 + share < ntiles ? t0 + share : ntiles;
  const uint64_t slot_of_group = (uint64_t)J.axis * gridDim.x + blockIdx.x;
  unsigned long long counted = 0;                                                // count pass, lane 0 of every wavefront
  uint64_t at = WRITE && slot_of_group ? J.block[slot_of_group - 1] : 0;         // write pass: the projections before this tile
  for (uint64_t t = t0; t < t1; ++t) {
    const uint64_t g0 = t * T;
    const uint32_t cnt = (uint32_t)(C - g0 < T ? C - g0 : T);
    lift_tile_heads(J.W, J.cap, J.first, J.F, g0, cnt, l_hs, l_hreg, l_ha, l_hbase, l_wave[0], l_span);
    uint32_t hs[ITEMS], v[ITEMS], e[ITEMS];
    uint64_t votes[ITEMS];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      const uint32_t slot = (uint32_t)j * TB + threadIdx.x;
      bool made = false;
      hs[j] = NONE32, v[j] = 0, e[j] = 0;
      if (slot < cnt) {
        hs[j] = l_hs[slot];
        const uint32_t p = l_hbase[hs[j]] + slot;
        e[j] = J.E[p];
        v[j] = J.V[p];
        if (e[j] > l_ha[hs[j]] && (!J.set || (v[j] & KEPT_BIT))) {  // a hit of the set; an empty other side makes no interval
          const uint32_t rec = v[j] & ~KEPT_BIT;
          made = J.c.end[J.axis ^ 1][rec] > J.c.start[J.axis ^ 1][rec];
        }
      }
      votes[j] = __ballot(made);
      if (!WRITE) counted += __popcll(votes[j]);
      else if (lane == 0) l_wave[j][wave] = (uint32_t)__popcll(votes[j]);
    }
    if (WRITE) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < ITEMS; ++j) {
        for (int w = 0; w < wave; ++w) at += l_wave[j][w];
        if (votes[j] >> lane & 1ull) {
          const uint64_t to = at + __popcll(votes[j] & ((1ull << lane) - 1ull));
          const swg_lift_region g = J.F[l_hreg[hs[j]]];
          const uint32_t rec = v[j] & ~KEPT_BIT, ax = J.axis, s1 = e[j];
          const uint32_t s0 = J.c.start[ax][rec], d0 = J.c.start[ax ^ 1][rec], d1 = J.c.end[ax ^ 1][rec];
          const bool minus = J.c.strand[rec] != 0;
          const uint32_t ca = g.start > s0 ? g.start : s0, cb = g.end < s1 ? g.end : s1;
          const uint64_t L = s1 - s0, D = d1 - d0;  // L > 0: a hit
          const uint64_t f0 = (uint64_t)(ca - s0) * D / L, c1 = ((uint64_t)(cb - s0) * D + L - 1) / L;
          const uint32_t from = minus ? d1 - (uint32_t)c1 : d0 + (uint32_t)f0, upto = minus ? d1 - (uint32_t)f0 : d0 + (uint32_t)c1;
          const uint64_t key = ((uint64_t)g.reserved << J.sb) | J.c.id[ax ^ 1][rec];
          if (to < J.n_proj)  // (always: the count pass counted these)
            *reinterpret_cast<uint4*>(J.proj + to) = make_uint4((uint32_t)key, (uint32_t)(key >> 32), from, upto);
        }
        for (int w = wave; w < WAVES; ++w) at += l_wave[j][w];
      }
    }
    __syncthreads();  // (LDS is reused by the next tile)
  }
  if (!WRITE) {
    if (threadIdx.x == 0) l_span[0] = 0;  // (the count of a share can pass 2^32: summed in 64 bits)
    __syncthreads();
    if (lane == 0 && counted) atomicAdd(reinterpret_cast<unsigned long long*>(&l_span[0]), counted);
    __syncthreads();
    if (threadIdx.x == 0) J.block[slot_of_group] = l_span[0];
  }
}

__global__ __launch_bounds__(TB) void closure_count_kernel(ClosureJoin J) { closure_tiles<false>(J); }
__global__ __launch_bounds__(TB) void closure_project_kernel(ClosureJoin J) { closure_tiles<true>(J); }

__global__ void closure_totals_kernel(const uint64_t* __restrict__ W0, const uint64_t* __restrict__ W1, uint64_t cap, const uint64_t* __restrict__ block,
                                      uint64_t n_block, unsigned long long* __restrict__ scalars) {
  if (threadIdx.x == 0) scalars[D_CAND] = W0 ? W0[cap - 1] : 0;
  if (threadIdx.x == 1) scalars[D_CAND + 1] = W1 ? W1[cap - 1] : 0;
  if (threadIdx.x == 2) scalars[D_PROJ] = block[n_block - 1];
}

// interval i < n_proj is projection i, the others are the visited pieces: events 2 i (start) and 2 i + 1 (end)
__global__ __launch_bounds__(TB) void closure_events_kernel(uint64_t n_proj, const ClosureProj* __restrict__ proj, uint64_t n_vis,
                                                            const swg_lift_region* __restrict__ vis, int sb, uint64_t* __restrict__ key,
                                                            uint64_t* __restrict__ pos) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_proj + n_vis) return;
  uint64_t k, s, e;
  const bool is_p = i < n_proj;
  if (is_p) {
    const ClosureProj p = proj[i];
    k = p.key, s = p.start, e = p.end;
  } else {
    const swg_lift_region g = vis[i - n_proj];
    k = ((uint64_t)g.reserved << sb) | g.seq, s = g.start, e = g.end;
  }
  key[2 * i] = key[2 * i + 1] = k;
  pos[2 * i] = s << 2 | (is_p ? 1u : 0u);
  pos[2 * i + 1] = e << 2 | (is_p ? 2u : 3u);
}

__global__ __launch_bounds__(TB) void closure_iota_kernel(uint64_t n, const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t* __restrict__ val) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  out[i] = in[i];
  val[i] = (uint32_t)i;
}

__global__ __launch_bounds__(TB) void closure_gather_kernel(uint64_t n, const uint64_t* __restrict__ in, const uint32_t* __restrict__ val,
                                                            uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i < n) out[i] = in[val[i]];
}

__global__ __launch_bounds__(TB) void closure_deltas_kernel(uint64_t n, const uint64_t* __restrict__ pos, const uint32_t* __restrict__ val,
                                                            uint64_t* __restrict__ delta, uint32_t* __restrict__ at) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint64_t p = pos[val[i]];
  const uint32_t kind = (uint32_t)p & 3u;
  delta[i] = kind == 0 ? V_ONE : kind == 1 ? 1ull : kind == 2 ? ~0ull : 0ull - V_ONE;
  at[i] = (uint32_t)(p >> 2);
}

__device__ __forceinline__ bool in_frontier(uint64_t depth) { return (uint32_t)depth != 0 && (depth >> 32) == 0; }

// Events at one position come as V starts, P starts, P ends, V ends.  Walking them one by one in that order, "in F" and "in V"
// change at most once between the state before the position and the state after it, and not at all when the two are equal (an end's
// interval was open before the position, so no depth passes through a value that neither side of the position has): every single
// event can be judged by the depths before and after it alone, and touching intervals never show a gap.
__global__ __launch_bounds__(TB) void closure_edges_kernel(uint64_t n, const uint64_t* __restrict__ depth, uint8_t* __restrict__ edge_f,
                                                           uint8_t* __restrict__ edge_v) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint64_t before = i ? depth[i - 1] : 0, after = depth[i];
  edge_f[i] = in_frontier(before) != in_frontier(after);
  edge_v[i] = (before != 0) != (after != 0);
}

__global__ __launch_bounds__(TB) void closure_pieces_kernel(uint64_t cap, const uint32_t* __restrict__ list, const uint64_t* __restrict__ key,
                                                            const uint32_t* __restrict__ at, int sb, swg_lift_region* __restrict__ out,
                                                            unsigned long long* __restrict__ scalars, int edges_slot, int count_slot) {
  const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const uint64_t pieces = scalars[edges_slot] >> 1;
  if (k == 0) scalars[count_slot] = pieces;
  if (k >= pieces || k >= cap) return;
  const uint32_t i0 = list[2 * k], i1 = list[2 * k + 1];
  const uint64_t kk = key[i0];
  out[k] = swg_lift_region{(uint32_t)(kk & ((uint64_t(1) << sb) - 1)), at[i0], at[i1], (uint32_t)(kk >> sb)};
}

__global__ __launch_bounds__(TB) void closure_rows_kernel(uint64_t count, const swg_lift_region* __restrict__ F, uint32_t hop, uint64_t off, int sb,
                                                          swg_closure_row* __restrict__ rows, uint64_t* __restrict__ key, uint64_t* __restrict__ pos) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= count) return;
  const swg_lift_region g = F[i];
  uint2* out = reinterpret_cast<uint2*>(rows + off + i);
  out[0] = make_uint2(g.reserved, g.seq);
  out[1] = make_uint2(g.start, g.end);
  out[2] = make_uint2(hop, 0u);
  key[off + i] = ((uint64_t)g.reserved << sb) | g.seq;
  pos[off + i] = g.start;
}

// The rows in (region, seq, start) order, and the summaries: runs of one region along the lanes are reduced first, one set of atomics
// per (wavefront, region).
__global__ __launch_bounds__(TB) void closure_finish_kernel(uint64_t n, const swg_closure_row* __restrict__ rows, const uint32_t* __restrict__ val,
                                                            swg_closure_row* __restrict__ out, swg_closure_summary* __restrict__ summary,
                                                            uint32_t max_hops, uint32_t min_len) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = i < n;
  uint32_t region = NONE32, seq = 0, start = 0, end = 0, hop = 0;
  bool new_seq = false;
  if (valid) {
    const uint2* in = reinterpret_cast<const uint2*>(rows + val[i]);
    const uint2 a = in[0], b = in[1], c = in[2];
    region = a.x, seq = a.y, start = b.x, end = b.y, hop = c.x;
    if (out) {
      uint2* o = reinterpret_cast<uint2*>(out + i);
      o[0] = a, o[1] = b, o[2] = c;
    }
    new_seq = true;
    if (i) {
      const uint2 before = reinterpret_cast<const uint2*>(rows + val[i - 1])[0];
      new_seq = before.x != region || before.y != seq;
    }
  }
  const uint32_t len = end - start;
  const bool cut = valid && hop == max_hops && len >= (min_len ? min_len : 1u);
  unsigned long long q[3] = {len, valid ? 1ull : 0ull, new_seq ? 1ull : 0ull};
  unsigned long long top = (unsigned long long)hop << 1 | (cut ? 1ull : 0ull);  // the largest hop and "cut" (which only the largest hop, max_hops, can set)
  const uint32_t left = __shfl_up(region, 1);
  const bool first_lane = lane == 0 || region != left;
  const int run_to = run_end(__ballot(first_lane), lane);
  run_sum(q, lane, run_to);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_down(top, d);
    if (lane + d < run_to && o > top) top = o;
  }
  if (first_lane && valid) {
    swg_closure_summary* s = summary + region;
    atomicAdd(reinterpret_cast<unsigned long long*>(&s->bases), q[0]);
    atomicAdd(&s->pieces, (uint32_t)q[1]);
    if (q[2]) atomicAdd(&s->sequences, (uint32_t)q[2]);
    atomicMax(&s->hops, (uint32_t)(top >> 1));
    if (top & 1ull) atomicOr(&s->flags, SWG_CLOSURE_CUT);
  }
}

int bad_input(swg_ctx* ctx, uint64_t bad) {
  if (bad & 1u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: a sequence id >= n_seq");
  if (bad & 2u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: a region with reserved != 0");
  if (bad & 4u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: a region with start > end");
  if (bad & 8u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: a region's seq is neither < n_seq nor UINT32_MAX");
  return SWG_OK;
}

unsigned blocks_of(uint64_t n) { return (unsigned)std::max<uint64_t>(1, (n + TB - 1) / TB); }

// The permutation that orders n elements by (key, pos), stable: two radix sorts, because the two together need more than 64 bits.
// On return *perm_out[i] is the element at sorted position i and *key_out[i] its key; pos and key are left as they are.  24 bytes
// of arena per element.
int sort_by_key_and_pos(swg_ctx* ctx, uint64_t n, const uint64_t* key, int key_bits, const uint64_t* pos, int pos_bits, uint32_t** perm_out,
                        uint64_t** key_out) {
  hipStream_t st = ctx->stream;
  uint64_t *a = swg_alloc<uint64_t>(ctx, n), *b = swg_alloc<uint64_t>(ctx, n);
  uint32_t *va = swg_alloc<uint32_t>(ctx, n), *vb = swg_alloc<uint32_t>(ctx, n);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "closure_iota", closure_iota_kernel<<<blocks_of(n), TB, 0, st>>>(n, pos, a, va));
  SWG_KERNEL_CHECK(ctx);
  {
    swg_prof_scope sort_scope(ctx, "closure_sort");
    SWG_TRY(swg_radix_sort_pairs(ctx, &a, &va, &b, &vb, n, 0, pos_bits));
  }
  SWG_LAUNCH(ctx, "closure_gather", closure_gather_kernel<<<blocks_of(n), TB, 0, st>>>(n, key, va, b));  // (b: the spare keys)
  SWG_KERNEL_CHECK(ctx);
  if (key_bits > 0) {
    swg_prof_scope sort_scope(ctx, "closure_sort");
    SWG_TRY(swg_radix_sort_pairs(ctx, &b, &va, &a, &vb, n, 0, key_bits));
  }
  *perm_out = va;
  *key_out = b;
  return SWG_OK;
}

struct Chunk {
  const swg_lift_region* pieces;
  uint64_t count;
  uint32_t hop;
};

// inside an arena frame; c and regions hold device pointers
int closure_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, const swg_lift_region* regions, uint64_t m, swg_closure_request* req) {
  hipStream_t st = ctx->stream;
  const uint32_t axes = req->axes, set = req->set, max_hops = req->max_hops, min_len = req->min_len;
  const int sb = swg_bits_for(n_seq), ob = swg_bits_for(m - 1);
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  swg_closure_summary* summary = swg_alloc<swg_closure_summary>(ctx, m);
  swg_lift_region* seed = swg_alloc<swg_lift_region>(ctx, m);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  SWG_HIP(ctx, hipMemsetAsync(summary, 0, m * sizeof(swg_closure_summary), st));
  SWG_TRY(swg_lift_limits(ctx, n, n_seq, c, scalars));
  uint64_t h[D_TOTAL];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_NF));
  SWG_TRY(bad_input(ctx, h[D_BAD]));
  LiftIndex ix[2];
  for (uint32_t ax = 0; ax < 2; ++ax)
    if (axes >> ax & 1u) SWG_TRY(swg_lift_index_build(ctx, n, n_seq, c, ax, h[D_MAX_START + ax], &ix[ax]));
  {  // hop 0
    const swg_arena_mark mark = swg_arena_save(ctx);
    uint8_t* flags = swg_alloc<uint8_t>(ctx, m);
    uint32_t* list = swg_alloc<uint32_t>(ctx, m);
    SWG_CHECK_ARENA(ctx);
    SWG_LAUNCH(ctx, "closure_seed", closure_seed_kernel<<<blocks_of(m), TB, 0, st>>>(m, regions, n_seq, flags, scalars));
    SWG_KERNEL_CHECK(ctx);
    swg_flag_scan fs{};
    SWG_TRY(swg_flags_count(ctx, flags, m, &fs, reinterpret_cast<uint64_t*>(scalars + D_NF)));
    SWG_TRY(swg_flags_compact(ctx, fs, list));
    SWG_LAUNCH(ctx, "closure_seed_pieces", closure_seed_pieces_kernel<<<blocks_of(m), TB, 0, st>>>(m, list, regions, seed, scalars));
    SWG_KERNEL_CHECK(ctx);
    swg_arena_restore(ctx, mark);
  }
  const unsigned G = (unsigned)std::min<uint64_t>((uint64_t)ctx->num_cu * 8, 2048);  // work-groups of a join
  std::vector<Chunk> chunks{{seed, 0, 0}};
  const swg_lift_region *frontier = seed, *visited = seed;
  uint64_t cap = m, total_rows = 0, projections = 0, candidates[2] = {0, 0};
  uint32_t hops_run = 0;
  bool last_counted = false;
  for (uint32_t hop = 1; hop <= max_hops; ++hop) {
    uint64_t* W[2] = {nullptr, nullptr};
    uint32_t* first[2] = {nullptr, nullptr};
    uint64_t* block = swg_alloc<uint64_t>(ctx, 2 * (uint64_t)G);
    for (uint32_t ax = 0; ax < 2; ++ax) {
      if (!(axes >> ax & 1u)) continue;
      W[ax] = swg_alloc<uint64_t>(ctx, cap);
      first[ax] = swg_alloc<uint32_t>(ctx, cap);
    }
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(block, 0, 2 * (uint64_t)G * sizeof(uint64_t), st));
    auto join_of = [&](uint32_t ax) {
      ClosureJoin J{};
      J.cap = cap, J.F = frontier, J.W = W[ax], J.first = first[ax], J.V = ix[ax].V, J.E = ix[ax].E;
      J.axis = ax, J.set = set, J.sb = sb, J.c = c, J.block = block;
      return J;
    };
    for (uint32_t ax = 0; ax < 2; ++ax) {
      if (!W[ax]) continue;
      const LiftIndex& x = ix[ax];
      SWG_LAUNCH(ctx, "closure_ranges",
                 closure_ranges_kernel<<<blocks_of(cap), TB, 0, st>>>(cap, frontier, scalars, hop, min_len, n, x.keys, x.M, x.pb, x.max_start, W[ax], first[ax]));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, W[ax], W[ax], cap));
      SWG_LAUNCH(ctx, "closure_count", closure_count_kernel<<<G, TB, 0, st>>>(join_of(ax)));
      SWG_KERNEL_CHECK(ctx);
    }
    SWG_TRY(swg_inclusive_sum_scan_u64(ctx, block, block, 2 * (uint64_t)G));
    SWG_LAUNCH(ctx, "closure_totals", closure_totals_kernel<<<1, 64, 0, st>>>(W[0], W[1], cap, block, 2 * (uint64_t)G, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_EDGES));  // the hop's one read-back
    if (hop == 1) SWG_TRY(bad_input(ctx, h[D_BAD]));                                    // (the regions' faults: closure_seed)
    const uint64_t n_front = h[D_NF], n_vis = h[D_NV], n_proj = h[D_PROJ];
    chunks.back().count = n_front;
    total_rows += n_front;
    last_counted = true;
    if (n_front == 0) break;  // nothing left to walk from
    hops_run = hop;
    projections += n_proj;
    candidates[0] += h[D_CAND], candidates[1] += h[D_CAND + 1];
    if (n_proj == 0) break;   // P_h is empty, and so is F_h
    const uint64_t n_iv = n_proj + n_vis, n_ev = 2 * n_iv;
    if (n_iv >= (uint64_t(1) << 30)) return swg_set_error(ctx, SWG_ERR_RANGE, "lift closure: 2^30 intervals or more in the union of hop %u", hop);
    // F_h and V_h stay; what follows them is given back when the hop is done
    swg_lift_region *next_front = swg_alloc<swg_lift_region>(ctx, n_iv), *next_vis = swg_alloc<swg_lift_region>(ctx, n_iv);
    const swg_arena_mark mark = swg_arena_save(ctx);
    ClosureProj* proj = swg_alloc<ClosureProj>(ctx, n_proj);
    uint64_t *ev_key = swg_alloc<uint64_t>(ctx, n_ev), *ev_pos = swg_alloc<uint64_t>(ctx, n_ev);
    SWG_CHECK_ARENA(ctx);
    for (uint32_t ax = 0; ax < 2; ++ax) {
      if (!W[ax]) continue;
      ClosureJoin J = join_of(ax);
      J.proj = proj, J.n_proj = n_proj;
      SWG_LAUNCH(ctx, "closure_project", closure_project_kernel<<<G, TB, 0, st>>>(J));
      SWG_KERNEL_CHECK(ctx);
    }
    SWG_LAUNCH(ctx, "closure_events", closure_events_kernel<<<blocks_of(n_iv), TB, 0, st>>>(n_proj, proj, n_vis, visited, sb, ev_key, ev_pos));
    SWG_KERNEL_CHECK(ctx);
    uint32_t* perm = nullptr;
    uint64_t* sorted_key = nullptr;
    SWG_TRY(sort_by_key_and_pos(ctx, n_ev, ev_key, sb + ob, ev_pos, 34, &perm, &sorted_key));
    uint64_t* depth = swg_alloc<uint64_t>(ctx, n_ev);
    uint32_t* at = swg_alloc<uint32_t>(ctx, n_ev);
    uint8_t* edge[2] = {swg_alloc<uint8_t>(ctx, n_ev), swg_alloc<uint8_t>(ctx, n_ev)};
    uint32_t* list[2] = {swg_alloc<uint32_t>(ctx, n_ev), swg_alloc<uint32_t>(ctx, n_ev)};
    SWG_CHECK_ARENA(ctx);
    SWG_LAUNCH(ctx, "closure_deltas", closure_deltas_kernel<<<blocks_of(n_ev), TB, 0, st>>>(n_ev, ev_pos, perm, depth, at));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_inclusive_sum_scan_u64(ctx, depth, depth, n_ev));
    SWG_LAUNCH(ctx, "closure_edges", closure_edges_kernel<<<blocks_of(n_ev), TB, 0, st>>>(n_ev, depth, edge[0], edge[1]));
    SWG_KERNEL_CHECK(ctx);
    swg_lift_region* const dst[2] = {next_front, next_vis};
    for (int k = 0; k < 2; ++k) {
      swg_flag_scan fs{};
      SWG_TRY(swg_flags_count(ctx, edge[k], n_ev, &fs, reinterpret_cast<uint64_t*>(scalars + D_EDGES + k)));
      SWG_TRY(swg_flags_compact(ctx, fs, list[k]));
      SWG_LAUNCH(ctx, "closure_pieces",
                 closure_pieces_kernel<<<blocks_of(n_iv), TB, 0, st>>>(n_iv, list[k], sorted_key, at, sb, dst[k], scalars, D_EDGES + k, k ? D_NV : D_NF));
      SWG_KERNEL_CHECK(ctx);
    }
    swg_arena_restore(ctx, mark);
    chunks.push_back(Chunk{next_front, 0, hop});
    last_counted = false;
    frontier = next_front, visited = next_vis, cap = n_iv;
  }
  if (!last_counted) {  // max_hops ended the walk: the size of the last frontier
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_NF), h, 1));
    chunks.back().count = h[0];
    total_rows += h[0];
  }
  if (total_rows >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "lift closure: 2^31 rows or more");
  if (total_rows) {
    swg_closure_row* rows = swg_alloc<swg_closure_row>(ctx, total_rows);
    uint64_t *key = swg_alloc<uint64_t>(ctx, total_rows), *pos = swg_alloc<uint64_t>(ctx, total_rows);
    const bool fetch = req->rows && total_rows <= req->capacity;
    swg_closure_row* sorted = fetch ? swg_alloc<swg_closure_row>(ctx, total_rows) : nullptr;
    SWG_CHECK_ARENA(ctx);
    uint64_t off = 0;
    for (const Chunk& k : chunks) {
      if (!k.count) continue;
      SWG_LAUNCH(ctx, "closure_rows", closure_rows_kernel<<<blocks_of(k.count), TB, 0, st>>>(k.count, k.pieces, k.hop, off, sb, rows, key, pos));
      SWG_KERNEL_CHECK(ctx);
      off += k.count;
    }
    uint32_t* perm = nullptr;
    uint64_t* sorted_key = nullptr;
    SWG_TRY(sort_by_key_and_pos(ctx, total_rows, key, sb + ob, pos, 32, &perm, &sorted_key));
    SWG_LAUNCH(ctx, "closure_finish", closure_finish_kernel<<<blocks_of(total_rows), TB, 0, st>>>(total_rows, rows, perm, sorted, summary, max_hops, min_len));
    SWG_KERNEL_CHECK(ctx);
    if (fetch) SWG_HIP(ctx, hipMemcpyAsync(req->rows, sorted, total_rows * sizeof(swg_closure_row), hipMemcpyDeviceToHost, st));
  }
  if (req->summary) SWG_HIP(ctx, hipMemcpyAsync(req->summary, summary, m * sizeof(swg_closure_summary), hipMemcpyDeviceToHost, st));
  SWG_HIP(ctx, hipStreamSynchronize(st));
  req->n = total_rows;
  req->hops_run = hops_run;
  req->projections = projections;
  req->candidates[0] = candidates[0], req->candidates[1] = candidates[1];
  return SWG_OK;
}

int hop0_only(swg_ctx* ctx, const swg_lift_region* regions, uint64_t m, uint32_t n_seq, swg_closure_request* req) {
  return bad_input(ctx, swg_closure_hop0_host(regions, m, n_seq, req));
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                swg_closure_request* req) {
  try {
    return swg_lift_closure_run(ctx, rec, on_device, status, regions, m, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

// the seams' argument checks, then the device work inside an arena frame (also the device half of swg_paf_lift_closure, host/lift_text.cpp)
int swg_lift_closure_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                         swg_closure_request* req) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: NULL records or request");
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: set must be SWG_IV_ALL or SWG_IV_KEPT");
  if (req->axes == 0 || req->axes >> 2) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: axes names nothing, or a bit beyond the two");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: the request's reserved word is not 0");
  if (req->max_hops == 0 || req->max_hops > 65535u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: max_hops must be 1 .. 65535");
  if (req->set == SWG_IV_KEPT && !status) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: the KEPT set needs a status column");
  if (m && !regions) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: NULL regions");
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "lift closure: 2^31 records or more in one call");
  if (m >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "lift closure: 2^31 regions or more in one call");
  req->n = req->projections = 0;
  req->hops_run = 0;
  req->candidates[0] = req->candidates[1] = 0;
  if (m == 0) return SWG_OK;
  if (n == 0) {  // no kernel: hop 0 is all there is
    if (!on_device) return hop0_only(ctx, regions, m, n_seq, req);
    std::vector<swg_lift_region> host(m);
    SWG_HIP(ctx, hipSetDevice(ctx->device));
    SWG_HIP(ctx, hipMemcpy(host.data(), regions, m * sizeof(swg_lift_region), hipMemcpyDeviceToHost));
    return hop0_only(ctx, host.data(), m, n_seq, req);
  }
  if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand)
    return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: NULL column (q_id, t_id, the four coordinates and strand are read)");
  if (n_seq == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "lift closure: records without sequences");
  if (!on_device)  // the regions are here: their faults cost no device work
    for (uint64_t r = 0; r < m; ++r)
      SWG_TRY(bad_input(ctx, (regions[r].reserved != 0 ? 2u : 0u) | (regions[r].start > regions[r].end ? 4u : 0u) |
                                 (regions[r].seq >= n_seq && regions[r].seq != UNKNOWN_SEQ ? 8u : 0u)));
  const int n_axes = __builtin_popcount(req->axes);
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * (24 * n_axes + (on_device ? 0 : 26)) + (size_t)m * (12 * n_axes + 400) + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const swg_lift_region* d_regions = regions;
    if (!on_device) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&c.id[0], &c.id[1], &c.start[0], &c.start[1], &c.end[0], &c.end[1]}) s.add(col, n);
      s.add(&c.strand, n);
      s.add(&c.status, n);
      s.add(&d_regions, m);
      SWG_TRY(s.run());
    }
    return closure_device(ctx, n, n_seq, c, d_regions, m, req);
  });
}

extern "C" int swg_lift_closure_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                        swg_closure_request* req) {
  return records_abi(ctx, rec, false, status, regions, m, req);
}

extern "C" int swg_lift_closure_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                               swg_closure_request* req) {
  return records_abi(ctx, rec, true, status, regions, m, req);
}
