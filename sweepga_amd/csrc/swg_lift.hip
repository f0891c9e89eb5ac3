// Lift: caller-given regions projected through the mappings.  An interval join: a small set of regions
// against the records sorted by (sequence, start) of one axis.  The work per region is unknown in advance and wildly uneven, so
// nothing here is "one thread (or wavefront, or work-group) per region": the regions' candidates are laid end to end in one
// stream and the stream is cut into tiles of T candidates.  Per wanted axis:
//
//   lift_limits     one pass over the records: ids out of range (the error word), the largest start of a record of non-zero length
//                   per axis.  Read back once, for both axes: it sizes the sort key.
//   lift_keys       key = seq << pb | s0 (pb = bits of the largest start), records of zero length get the sentinel sequence n_seq;
//                   value = record | KEPT_BIT when status != 0: ALL and KEPT come from ONE index and one candidate pass.
//   (sort)          swg_radix_sort_pairs over pb + bits(n_seq) key bits; stable: equal keys stay in record order
//   lift_gather     E[p] = the end of the record at sorted position p, M[p] = seq << 32 | end -- into the sort's spare pair
//   (scan)          swg_inclusive_max_scan_u64 over M: the sequence in the high half makes it a per-sequence prefix maximum
//   lift_ranges     one thread per region: hi = the first position with s0 >= b (binary search on the keys), p0 = the first
//                   position of the sequence whose prefix maximum of ends exceeds a (binary search on M, monotone).  Every hit
//                   lies in [p0, hi), and a candidate there is a hit iff its own end > a.  w = hi - p0 (0 for an empty or unknown
//                   region); the regions' own faults go to the error word.
//   (scan)          swg_inclusive_sum_scan_u64 over w: the candidate stream of C = sum(w) items.  C is read back: it sizes the grid.
//   lift_count      a tile of T candidates per work-group step: the regions the tile spans from two binary searches in the scanned
//                   offsets, their heads expanded in LDS (regions without candidates are walked over, never expanded), a running
//                   maximum of the head slots gives every slot its region.  Each lane tests its candidates; runs of one region
//                   along the lanes are summed first, then go to the region's LDS counters, and one global atomic per (work-group,
//                   region touched, counter) reaches hits[set][axis].  The tile's row count is stored.
//   (scan)          swg_inclusive_sum_scan_u64 over the tile counts.  With both axes, the per-region counts of the other axis are
//                   scanned too: a region's rows of axis 0 come before its rows of axis 1.
//   lift_rows       only when the caller's capacity holds the rows: the same tile again, ranks from wavefront ballots and the
//                   work-group's wave counts (flag_compact's scheme), every row written as two 16-byte stores at tile offset +
//                   rank + the other axis' share: the rows come out in (region, axis, s0, record) order without a sort.
//
// No work-group waits for another inside a launch; every carry goes through the library's scans between launches.
//
// The index (lift_limits, lift_keys, the sort, lift_gather, the prefix maximum) is built by swg_lift_limits / swg_lift_index_build,
// which swg_lift_index.h declares with the device side of a join (lift_candidates, lift_tile_heads): the transitive lift
// (swg_lift_closure.hip) builds it once and joins every hop's frontier against it.
#include <algorithm>
#include <cstring>
#include <new>

#include "swg_internal.h"
#include "swg_lift_index.h"
#include "swg_pair_table.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;
using namespace swg_lift_ix;
// device scalars after lift_limits' (swg_lift_index.h): the rows per axis
enum { D_ROWS = 3, D_TOTAL = 5 };

__global__ __launch_bounds__(TB) void lift_limits_kernel(uint64_t n, uint32_t n_seq, LiftCols c, unsigned long long* __restrict__ scalars) {
  __shared__ unsigned long long l_max[2][WAVES];
  unsigned long long mx[2] = {0, 0};
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TB) {
    bad |= c.id[0][i] >= n_seq || c.id[1][i] >= n_seq;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
      const uint32_t s = c.start[ax][i];
      if (c.end[ax][i] > s && s > mx[ax]) mx[ax] = s;
    }
  }
  if (bad) atomicOr(&scalars[D_BAD], 1ull);
#pragma unroll
  for (int ax = 0; ax < 2; ++ax) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_down(mx[ax], d);
      if (o > mx[ax]) mx[ax] = o;
    }
    if ((threadIdx.x & 63) == 0) l_max[ax][threadIdx.x >> 6] = mx[ax];
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long m = 0;
    for (int w = 0; w < WAVES; ++w) m = l_max[threadIdx.x][w] > m ? l_max[threadIdx.x][w] : m;
    if (m) atomicMax(&scalars[D_MAX_START + threadIdx.x], m);
  }
}

__global__ __launch_bounds__(TB) void lift_keys_kernel(uint64_t n, uint32_t n_seq, const uint32_t* __restrict__ id, const uint32_t* __restrict__ start,
                                                       const uint32_t* __restrict__ end, const uint8_t* __restrict__ status, int pb,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = start[i];
  const bool live = end[i] > s;  // (ids are in range: lift_limits has looked)
  keys[i] = live ? ((uint64_t)id[i] << pb) | s : (uint64_t)n_seq << pb;
  vals[i] = (uint32_t)i | (status && status[i] != 0 ? KEPT_BIT : 0u);
}

__global__ __launch_bounds__(TB) void lift_gather_kernel(uint64_t n, uint32_t n_seq, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ end, int pb, uint32_t* __restrict__ E,
                                                         uint64_t* __restrict__ M) {
  const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (p >= n) return;
  const uint64_t seq = keys[p] >> pb;
  const uint32_t e = seq < n_seq ? end[vals[p] & ~KEPT_BIT] : 0u;
  E[p] = e;
  M[p] = (seq << 32) | e;
}

__global__ __launch_bounds__(TB) void lift_ranges_kernel(uint64_t m, const swg_lift_region* __restrict__ regions, uint64_t n, uint32_t n_seq,
                                                         const uint64_t* __restrict__ keys, const uint64_t* __restrict__ M, int pb, uint64_t max_start,
                                                         uint64_t* __restrict__ w, uint32_t* __restrict__ first, unsigned long long* __restrict__ scalars) {
  const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (r >= m) return;
  const swg_lift_region g = regions[r];
  unsigned long long bad = 0;
  if (g.reserved != 0) bad |= 2ull;
  if (g.start > g.end) bad |= 4ull;
  if (g.seq >= n_seq && g.seq != UNKNOWN_SEQ) bad |= 8ull;
  uint64_t width = 0;
  uint32_t p0 = 0;
  if (bad) {
    atomicOr(&scalars[D_BAD], bad);
  } else if (g.seq != UNKNOWN_SEQ && g.start < g.end) {
    width = lift_candidates(n, keys, M, pb, max_start, g.seq, g.start, g.end, &p0);
  }
  w[r] = width;
  first[r] = p0;
}

struct LiftJoin {
  uint64_t m, C, ntiles;
  const swg_lift_region* regions;
  const uint64_t* W;      // [m] inclusive scan of the widths
  const uint32_t* first;  // [m] p0
  const uint32_t *V, *E;  // the index: values and ends in sorted order
  uint32_t axis, set;
  uint32_t* summary;      // [m][2][2]
  uint64_t* tile;         // [ntiles]: count pass: the tile's rows; write pass: their inclusive scan
  const uint64_t* other;  // [m] inclusive scan of the other axis' rows per region, or nullptr (one axis)
  LiftCols c;
  swg_lift_row* rows;
  uint64_t n_rows;
};

__device__ __forceinline__ void lift_row(const LiftJoin& J, uint32_t r, uint32_t v, uint32_t s1, uint64_t at) {
  const uint32_t rec = v & ~KEPT_BIT, ax = J.axis;
  const swg_lift_region g = J.regions[r];
  const uint32_t s0 = J.c.start[ax][rec], d0 = J.c.start[ax ^ 1][rec], d1 = J.c.end[ax ^ 1][rec];
  const uint32_t minus = J.c.strand[rec] != 0 ? 1u : 0u;
  const uint32_t ca = g.start > s0 ? g.start : s0, cb = g.end < s1 ? g.end : s1;
  const uint64_t L = s1 - s0, D = d1 - d0;  // L > 0: a hit
  const uint64_t f0 = (uint64_t)(ca - s0) * D / L, c1 = ((uint64_t)(cb - s0) * D + L - 1) / L;
  const uint32_t from = minus ? d1 - (uint32_t)c1 : d0 + (uint32_t)f0, to = minus ? d1 - (uint32_t)f0 : d0 + (uint32_t)c1;
  uint4* out = reinterpret_cast<uint4*>(J.rows + at);
  out[0] = make_uint4(r, rec, ca, cb);
  out[1] = make_uint4(J.c.id[ax ^ 1][rec], from, to, minus | (ax << 1));
}

template <bool WRITE>
__device__ __forceinline__ void lift_tiles(const LiftJoin& J) {
  __shared__ uint32_t l_hs[T];      // per slot: the slot where its region begins in this tile (after the scan)
  __shared__ uint32_t l_hreg[T];    // per head slot: the region, its start, and (p0 - head slot) mod 2^32: position = base + slot
  __shared__ uint32_t l_ha[T];
  __shared__ uint32_t l_hbase[T];
  __shared__ uint32_t l_cnt[2][T];  // per head slot: the hits of ALL and KEPT (count pass)
  __shared__ uint32_t l_wave[ITEMS][WAVES];
  __shared__ uint64_t l_span[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t t = blockIdx.x; t < J.ntiles; t += gridDim.x) {
    const uint64_t g0 = t * T;
    const uint32_t cnt = (uint32_t)(J.C - g0 < T ? J.C - g0 : T);
    if (!WRITE)
      for (int s = threadIdx.x; s < T; s += TB) l_cnt[0][s] = l_cnt[1][s] = 0;
    lift_tile_heads(J.W, J.m, J.first, J.regions, g0, cnt, l_hs, l_hreg, l_ha, l_hbase, l_wave[0], l_span);
    // the candidates: striped, slot = j * TB + thread
    uint32_t hs[ITEMS], v[ITEMS], e[ITEMS];
    uint64_t votes[ITEMS];
    unsigned long long rows_here = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      const uint32_t slot = (uint32_t)j * TB + threadIdx.x;
      const bool valid = slot < cnt;
      bool hit = false, kept = false;
      hs[j] = NONE32, v[j] = 0, e[j] = 0;
      if (valid) {
        hs[j] = l_hs[slot];
        const uint32_t p = l_hbase[hs[j]] + slot;
        e[j] = J.E[p];
        v[j] = J.V[p];
        hit = e[j] > l_ha[hs[j]];
        kept = hit && (v[j] & KEPT_BIT);
      }
      const bool row = J.set ? kept : hit;
      votes[j] = __ballot(row);
      if (!WRITE) {
        // runs of one region along the lanes, summed towards the run's first lane
        unsigned long long q[2] = {hit ? 1ull : 0ull, kept ? 1ull : 0ull};
        const uint32_t left = __shfl_up(hs[j], 1);
        const bool first_lane = lane == 0 || hs[j] != left;
        run_sum(q, lane, run_end(__ballot(first_lane), lane));
        if (first_lane && valid) {
          if (q[0]) atomicAdd(&l_cnt[0][hs[j]], (uint32_t)q[0]);
          if (q[1]) atomicAdd(&l_cnt[1][hs[j]], (uint32_t)q[1]);
        }
        if (lane == 0) rows_here += __popcll(votes[j]);
      } else if (lane == 0) {
        l_wave[j][wave] = (uint32_t)__popcll(votes[j]);
      }
    }
    if (!WRITE) {
      if (lane == 0) l_wave[0][wave] = (uint32_t)rows_here;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint64_t total = 0;
        for (int w = 0; w < WAVES; ++w) total += l_wave[0][w];
        J.tile[t] = total;
      }
      for (uint32_t s = threadIdx.x; s < cnt; s += TB) {  // one atomic per (region touched, counter)
        if (l_hs[s] != s) continue;
        uint32_t* out = J.summary + (uint64_t)l_hreg[s] * 4 + J.axis;
        if (l_cnt[0][s]) atomicAdd(out, l_cnt[0][s]);
        if (l_cnt[1][s]) atomicAdd(out + 2, l_cnt[1][s]);
      }
    } else {
      __syncthreads();
      uint64_t at = t ? J.tile[t - 1] : 0;  // rows of the tiles before this one
#pragma unroll
      for (int j = 0; j < ITEMS; ++j) {
        for (int w = 0; w < wave; ++w) at += l_wave[j][w];
        if (votes[j] >> lane & 1ull) {
          const uint32_t r = l_hreg[hs[j]];
          uint64_t to = at + __popcll(votes[j] & ((1ull << lane) - 1ull));
          if (J.other) to += J.axis ? J.other[r] : (r ? J.other[r - 1] : 0);  // a region's rows of axis 0 come before those of axis 1
          if (to < J.n_rows) lift_row(J, r, v[j], e[j], to);  // (always: the count pass counted these rows)
        }
        for (int w = wave; w < WAVES; ++w) at += l_wave[j][w];
      }
    }
    __syncthreads();  // (LDS is reused by the next tile)
  }
}

__global__ __launch_bounds__(TB) void lift_count_kernel(LiftJoin J) { lift_tiles<false>(J); }
__global__ __launch_bounds__(TB) void lift_rows_kernel(LiftJoin J) { lift_tiles<true>(J); }

__global__ __launch_bounds__(TB) void lift_region_rows_kernel(uint64_t m, const uint32_t* __restrict__ summary, uint32_t set, uint32_t axis,
                                                              uint64_t* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (r < m) out[r] = summary[r * 4 + set * 2 + axis];
}

__global__ void lift_totals_kernel(const uint64_t* __restrict__ tile0, uint64_t ntiles0, const uint64_t* __restrict__ tile1, uint64_t ntiles1,
                                   unsigned long long* __restrict__ scalars) {
  if (threadIdx.x == 0) scalars[D_ROWS] = ntiles0 ? tile0[ntiles0 - 1] : 0;
  if (threadIdx.x == 1) scalars[D_ROWS + 1] = ntiles1 ? tile1[ntiles1 - 1] : 0;
}

// one axis of a lift call: the index, and the candidate stream of the call's regions over it
struct AxisIndex : LiftIndex {
  uint64_t *W = nullptr, *tile = nullptr;
  uint32_t* first = nullptr;
  uint64_t C = 0, ntiles = 0;
};

int bad_input(swg_ctx* ctx, uint64_t bad) {
  if (bad & 1u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: a sequence id >= n_seq");
  if (bad & 2u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: a region with reserved != 0");
  if (bad & 4u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: a region with start > end");
  if (bad & 8u) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: a region's seq is neither < n_seq nor UINT32_MAX");
  return SWG_OK;
}

// inside an arena frame; c and regions hold device pointers.  dev: the finished rows stay in the frame for the caller (the exact
// lift and the hit records, swg_cigar.hip) instead of going to req->rows
int lift_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, const swg_lift_region* regions, uint64_t m, swg_lift_request* req,
                LiftDeviceRows* dev = nullptr) {
  hipStream_t st = ctx->stream;
  const uint32_t axes = req->axes, set = req->set;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  uint32_t* summary = swg_alloc<uint32_t>(ctx, m * 4);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  SWG_HIP(ctx, hipMemsetAsync(summary, 0, m * 4 * sizeof(uint32_t), st));
  SWG_TRY(swg_lift_limits(ctx, n, n_seq, c, scalars));
  uint64_t h[D_TOTAL];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_ROWS));
  SWG_TRY(bad_input(ctx, h[D_BAD]));
  const unsigned grid_m = (unsigned)((m + TB - 1) / TB);
  AxisIndex ix[2];
  for (uint32_t ax = 0; ax < 2; ++ax) {
    if (!(axes >> ax & 1u)) continue;
    AxisIndex& x = ix[ax];
    SWG_TRY(swg_lift_index_build(ctx, n, n_seq, c, ax, h[D_MAX_START + ax], &x));
    x.W = swg_alloc<uint64_t>(ctx, m);
    x.first = swg_alloc<uint32_t>(ctx, m);
    SWG_CHECK_ARENA(ctx);
    SWG_LAUNCH(ctx, "lift_ranges", lift_ranges_kernel<<<grid_m, TB, 0, st>>>(m, regions, n, n_seq, x.keys, x.M, x.pb, x.max_start, x.W, x.first, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_inclusive_sum_scan_u64(ctx, x.W, x.W, m));
    SWG_TRY(swg_read_scalars(ctx, x.W + (m - 1), &x.C, 1));  // sizes the join's grid
    x.ntiles = (x.C + T - 1) / T;
    x.tile = swg_alloc<uint64_t>(ctx, x.ntiles ? x.ntiles : 1);
    SWG_CHECK_ARENA(ctx);
  }
  auto join_of = [&](uint32_t ax) {
    const AxisIndex& x = ix[ax];
    LiftJoin J{};
    J.m = m, J.C = x.C, J.ntiles = x.ntiles;
    J.regions = regions, J.W = x.W, J.first = x.first, J.V = x.V, J.E = x.E;
    J.axis = ax, J.set = set, J.summary = summary, J.tile = x.tile, J.c = c;
    return J;
  };
  auto grid_of = [&](const AxisIndex& x) { return (unsigned)std::min<uint64_t>(x.ntiles, (uint64_t)ctx->num_cu * 16); };
  for (uint32_t ax = 0; ax < 2; ++ax) {
    const AxisIndex& x = ix[ax];
    if (!x.ntiles) continue;
    SWG_LAUNCH(ctx, "lift_count", lift_count_kernel<<<grid_of(x), TB, 0, st>>>(join_of(ax)));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_inclusive_sum_scan_u64(ctx, x.tile, x.tile, x.ntiles));
  }
  SWG_LAUNCH(ctx, "lift_totals", lift_totals_kernel<<<1, 64, 0, st>>>(ix[0].tile, ix[0].ntiles, ix[1].tile, ix[1].ntiles, scalars));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  SWG_TRY(bad_input(ctx, h[D_BAD]));  // (the regions' faults: lift_ranges)
  const uint64_t n_rows = h[D_ROWS] + h[D_ROWS + 1];
  req->n = n_rows;
  req->candidates[0] = ix[0].C;
  req->candidates[1] = ix[1].C;
  if (req->summary) SWG_HIP(ctx, hipMemcpyAsync(req->summary, summary, m * sizeof(swg_lift_summary), hipMemcpyDeviceToHost, st));
  const bool fetch = req->rows && n_rows <= req->capacity;
  if (n_rows && (fetch || (dev && dev->always))) {
    swg_lift_row* rows = swg_alloc<swg_lift_row>(ctx, n_rows);
    uint64_t* other[2] = {nullptr, nullptr};  // other[ax]: the scanned rows per region of axis 1 - ax
    const bool both = h[D_ROWS] && h[D_ROWS + 1];
    if (both)
      for (auto& o : other) o = swg_alloc<uint64_t>(ctx, m);
    SWG_CHECK_ARENA(ctx);
    for (uint32_t ax = 0; ax < 2 && both; ++ax) {
      SWG_LAUNCH(ctx, "lift_region_rows", lift_region_rows_kernel<<<grid_m, TB, 0, st>>>(m, summary, set, ax ^ 1, other[ax]));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, other[ax], other[ax], m));
    }
    for (uint32_t ax = 0; ax < 2; ++ax) {
      if (!h[D_ROWS + ax]) continue;
      LiftJoin J = join_of(ax);
      J.other = other[ax], J.rows = rows, J.n_rows = n_rows;
      SWG_LAUNCH(ctx, "lift_rows", lift_rows_kernel<<<grid_of(ix[ax]), TB, 0, st>>>(J));
      SWG_KERNEL_CHECK(ctx);
    }
    if (dev) dev->rows = rows;
    else SWG_HIP(ctx, hipMemcpyAsync(req->rows, rows, n_rows * sizeof(swg_lift_row), hipMemcpyDeviceToHost, st));
  }
  SWG_HIP(ctx, hipStreamSynchronize(st));
  return SWG_OK;
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                swg_lift_request* req) {
  try {
    return swg_lift_run(ctx, rec, on_device, status, regions, m, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

int swg_lift_ix::swg_lift_limits(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, unsigned long long* scalars) {
  SWG_LAUNCH(ctx, "lift_limits", lift_limits_kernel<<<grid_for(ctx, n), TB, 0, ctx->stream>>>(n, n_seq, c, scalars));
  SWG_KERNEL_CHECK(ctx);
  return SWG_OK;
}

int swg_lift_ix::swg_lift_index_build(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, uint32_t ax, uint64_t max_start, LiftIndex* out) {
  hipStream_t st = ctx->stream;
  LiftIndex& x = *out;
  const unsigned grid_n = (unsigned)((n + TB - 1) / TB);
  const int pb = swg_bits_for(max_start);
  x.max_start = max_start, x.pb = pb;
  x.keys = swg_alloc<uint64_t>(ctx, n);
  x.M = swg_alloc<uint64_t>(ctx, n);
  x.V = swg_alloc<uint32_t>(ctx, n);
  x.E = swg_alloc<uint32_t>(ctx, n);
  SWG_CHECK_ARENA(ctx);
  SWG_LAUNCH(ctx, "lift_keys", lift_keys_kernel<<<grid_n, TB, 0, st>>>(n, n_seq, c.id[ax], c.start[ax], c.end[ax], c.status, pb, x.keys, x.V));
  SWG_KERNEL_CHECK(ctx);
  {
    swg_prof_scope sort_scope(ctx, "lift_sort");
    SWG_TRY(swg_radix_sort_pairs(ctx, &x.keys, &x.V, &x.M, &x.E, n, 0, pb + swg_bits_for(n_seq)));  // (the spare pair: M and E)
  }
  SWG_LAUNCH(ctx, "lift_gather", lift_gather_kernel<<<grid_n, TB, 0, st>>>(n, n_seq, x.keys, x.V, c.end[ax], pb, x.E, x.M));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_inclusive_max_scan_u64(ctx, x.M, x.M, n));
  return SWG_OK;
}

int swg_lift_ix::swg_lift_rows_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, const swg_lift_region* regions, uint64_t m,
                                      swg_lift_request* req, LiftDeviceRows* dev) {
  return lift_device(ctx, n, n_seq, c, regions, m, req, dev);
}

int swg_lift_ix::swg_lift_check_request(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                        uint32_t set, uint32_t axes) {
  if (set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: set must be SWG_IV_ALL or SWG_IV_KEPT");
  if (axes == 0 || axes >> 2) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: axes names nothing, or a bit beyond the two");
  if (set == SWG_IV_KEPT && !status) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: the KEPT rows need a status column");
  if (m && !regions) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: NULL regions");
  if (rec->n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "lift: 2^31 records or more in one call");
  if (m >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "lift: 2^31 regions or more in one call");
  return SWG_OK;
}

int swg_lift_ix::swg_lift_check_columns(swg_ctx* ctx, const swg_records* rec, bool on_device, const swg_lift_region* regions, uint64_t m) {
  const uint32_t n_seq = rec->n_seq;
  if (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand)
    return swg_set_error(ctx, SWG_ERR_INVALID, "lift: NULL column (q_id, t_id, the four coordinates and strand are read)");
  if (n_seq == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: records without sequences");
  if (!on_device)  // the regions are here: their faults cost no device work
    for (uint64_t r = 0; r < m; ++r)
      SWG_TRY(bad_input(ctx, (regions[r].reserved != 0 ? 2u : 0u) | (regions[r].start > regions[r].end ? 4u : 0u) |
                                 (regions[r].seq >= n_seq && regions[r].seq != UNKNOWN_SEQ ? 8u : 0u)));
  return SWG_OK;
}

void swg_lift_ix::swg_lift_stage(swg_stager* s, uint64_t n, uint64_t m, LiftCols* c, const swg_lift_region** regions) {
  for (const uint32_t** col : {&c->id[0], &c->id[1], &c->start[0], &c->start[1], &c->end[0], &c->end[1]}) s->add(col, n);
  s->add(&c->strand, n);
  s->add(&c->status, n);
  s->add(regions, m);
}

// the seams' argument checks, then the device work inside an arena frame (also the device half of swg_paf_lift, host/lift_text.cpp)
int swg_lift_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                 swg_lift_request* req) {
  static_assert(sizeof(swg_lift_row) == 32 && sizeof(swg_lift_region) == 16 && sizeof(swg_lift_summary) == 16, "the ABI's sizes");
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "lift: NULL records or request");
  SWG_TRY(swg_lift_check_request(ctx, rec, status, regions, m, req->set, req->axes));
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  req->n = 0;
  req->candidates[0] = req->candidates[1] = 0;
  if (m == 0 || n == 0) {  // no device work
    if (req->summary && m) std::memset(req->summary, 0, m * sizeof(swg_lift_summary));
    return SWG_OK;
  }
  SWG_TRY(swg_lift_check_columns(ctx, rec, on_device, regions, m));
  const int n_axes = __builtin_popcount(req->axes);
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * (24 * n_axes + (on_device ? 0 : 26)) + (size_t)m * (12 * n_axes + 48) + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const swg_lift_region* d_regions = regions;
    if (!on_device) {
      swg_stager s(ctx);
      swg_lift_stage(&s, n, m, &c, &d_regions);
      SWG_TRY(s.run());
    }
    return lift_device(ctx, n, n_seq, c, d_regions, m, req);
  });
}

extern "C" int swg_lift_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                swg_lift_request* req) {
  return records_abi(ctx, rec, false, status, regions, m, req);
}

extern "C" int swg_lift_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                       swg_lift_request* req) {
  return records_abi(ctx, rec, true, status, regions, m, req);
}
