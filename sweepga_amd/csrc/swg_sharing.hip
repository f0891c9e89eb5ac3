// Sharing: how many genomes cover each base.  Breadth and intervals work per unit -- one sequence against
// one genome of the other side; this counts across the units of a sequence.  cover(s, g) is the union of the unit (s, g) over
// BOTH axes, depth(s, x) the number of genomes g with x in cover(s, g).  Per set (ALL records, KEPT records) the runs -- maximal
// stretches of one depth >= 1, ordered by (sequence, start) -- and the spectrum: bases of every genome's sequences at every depth.
//
//   sharing_keys          every record gives two entries: (segment(q, genome(t)) << 32 | q_start) at i and (segment(t, genome(q))
//                         << 32 | t_start) at n + i; value = record index | AXIS_FLAG | KEPT_FLAG.  Records that do not count get
//                         the sentinel segment.  SegMap and the hashed set: swg_union_tiles.h, as in breadth and intervals.
//   (sort)                swg_radix_sort_pairs over the 2n entries
//   sharing_gather        gather_tile<true, true, true>: end = (AXIS_FLAG ? t_end : q_end)[record] in sorted order and the tile
//                         maxima of P = segment << 32 | end over the entries of non-zero length, ALL and KEPT
//   (scan)                swg_inclusive_max_scan_u64 over the tile maxima of the sets asked for
//   sharing_count         heads per tile and set: heads_tile<false> of swg_union_tiles.h, the walk of intervals_count.  An entry is
//                         a head when nothing of its set and segment came before it or its start lies beyond the running maximum
//                         (touching intervals join)
//   (scan)                swg_exclusive_scan_u32 over the tile counts; the totals m are the merged intervals of each set.  Read back.
//   sharing_events        the tile again, heads_tile<true> with this file's emitter EventsOut: the head of rank r writes the event
//                         (seq << 32 | start, +1) at r and closes the interval before it: (seq' << 32 | end', -1) at m + r - 1, seq'
//                         and end' from the running maximum in front of it.  The last interval is closed from the last tile's
//                         scanned maximum.
// then per set:
//   (sort)                swg_radix_sort_pairs over the 2m events, 32 + bits(n_seq) key bits; the value is the delta
//   (scan)                swg_exclusive_scan_u32 over the deltas: the depth in front of every event.  The sums wrap; the deltas of a
//                         sequence cancel, so depth is 0 at every sequence's first event and nothing has to be segmented.  Inside
//                         a group of equal keys the order is arbitrary: only the depth in front of the group's first event and
//                         behind its last mean anything.
//   sharing_group_first   first[p] = p where a group begins, else 0; (scan) swg_inclusive_max_scan_u32 makes it every event's
//                         group begin.  (This replaces the compaction of the group-lasts: the depth behind the previous group is
//                         the depth in front of this group's first event.)
//   sharing_break_flags   flag[p] = p is its group's last event and the depth behind it differs from the depth in front of the
//                         group: a breakpoint.  A group where one genome's cover ends and another's begins is none.
//   (compaction)          swg_flags_count / swg_flags_compact: the breakpoints in (seq, position) order.  Read back their number.
//   sharing_open_flags    per breakpoint its key and the depth behind it, compactly; flag = that depth is not 0: it opens a run
//   (compaction)          the openers.  Read back their number: the runs.
//   sharing_runs          run j = {seq, position of its opener, position of the NEXT breakpoint, depth}.  Depth is 0 behind every
//                         sequence's last event, so the next breakpoint of an opener lies in the same sequence.
//   sharing_bases         sum(end - start) over the runs (runs bit)
//   sharing_spectrum      (spectrum bit) one pass over the runs: end - start added to (genome(seq), depth).  Equal keys along the
//                         lanes of a wavefront are summed first, the run heads go through the work-group's LDS table, one atomic
//                         per (work-group, key) reaches the device array (the scheme of swg_pair_table.h; DESIGN.md section 13 (3)
//                         has the reason).
//   sharing_lengths       (spectrum bit, seq_len given) seq_len[s] added to (genome(s), 0), same scheme
//   sharing_private       ... and the row's other entries taken off column 0
//
// No work-group waits for another inside a launch: every carry goes through the library's scans between launches.  No atomic
// touches a row, so the order is exact; the spectrum's integer sums do not depend on the order of their atomics.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;
using namespace swg_union_tiles;
// device scalars: bad input (bit 0: an id out of range, bit 1: a record ends beyond its sequence), the heads of ALL and KEPT, then
// per set the breakpoints, the runs and their bases
enum { D_BAD = 0, D_HEADS = 1, D_SET = 3, S_BREAKS = 0, S_RUNS = 1, S_BASES = 2, S_COUNT = 3, D_TOTAL = D_SET + 2 * S_COUNT };
constexpr uint32_t SET_ALL = 1u, SET_KEPT = 2u;
constexpr uint32_t WANT_RUNS = 0x3u, WANT_SPECTRUM = 0xcu;
constexpr uint32_t MAX_SPECTRUM_GENOMES = 4096;
using Spectrum = PairTable<1, false>;  // dense: slot = genome * G + depth

__global__ __launch_bounds__(TB) void sharing_keys_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                          const uint32_t* __restrict__ q_start, const uint32_t* __restrict__ t_start,
                                                          const uint32_t* __restrict__ q_end, const uint32_t* __restrict__ t_end,
                                                          const uint8_t* __restrict__ status, const uint32_t* __restrict__ seq_genome,
                                                          const uint32_t* __restrict__ seq_len, uint32_t n_seq, SegMap M,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          unsigned long long* __restrict__ scalars) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = q_id[i], t = t_id[i];
  const uint32_t gq = q < n_seq ? seq_genome[q] : NONE32, gt = t < n_seq ? seq_genome[t] : NONE32;
  uint64_t key_q = (uint64_t)M.sentinel << 32, key_t = key_q;
  if (gq >= M.G || gt >= M.G) {
    atomicOr(&scalars[D_BAD], 1ull);
  } else if (gq != gt) {
    const unsigned long long pq = (unsigned long long)q * M.G + gt, pt = (unsigned long long)t * M.G + gq;
    const uint32_t sq = M.set_keys ? table_slot(M.set_keys, M.set_mask, pq) : (uint32_t)pq;
    const uint32_t st = M.set_keys ? table_slot(M.set_keys, M.set_mask, pt) : (uint32_t)pt;
    key_q = ((uint64_t)sq << 32) | q_start[i];
    key_t = ((uint64_t)st << 32) | t_start[i];
    if (seq_len && (q_end[i] > seq_len[q] || t_end[i] > seq_len[t])) atomicOr(&scalars[D_BAD], 2ull);
  }
  const uint32_t v = (uint32_t)i | (status && status[i] != 0 ? KEPT_FLAG : 0u);
  keys[i] = key_q, vals[i] = v;
  keys[n + i] = key_t, vals[n + i] = v | AXIS_FLAG;
}

__global__ __launch_bounds__(TB) void sharing_gather_kernel(uint64_t n2, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            const uint32_t* __restrict__ q_end, const uint32_t* __restrict__ t_end,
                                                            uint32_t sentinel, uint32_t* __restrict__ ends,
                                                            unsigned long long* __restrict__ tile_max, uint64_t ntiles) {
  gather_tile<true, true, true>(n2, keys, vals, q_end, sentinel, ends, tile_max, ntiles, nullptr, t_end);
}

struct EventsOut {       // the write pass' emitter (heads_tile, swg_union_tiles.h): the events per set (ALL, KEPT)
  SegMap M;
  uint64_t* keys[2];     // [2 * total[s]]: seq << 32 | position; the begins at [0, total), the ends at [total, 2 * total)
  uint32_t* deltas[2];   // [2 * total[s]]: +1, -1
  uint32_t total[2];
  __device__ __forceinline__ void event(int s, uint64_t at, unsigned long long p, uint32_t delta) const {  // p = segment << 32 | position
    uint32_t seq, other;
    segment_of(M, (uint32_t)(p >> 32), &seq, &other);
    keys[s][at] = ((uint64_t)seq << 32) | (uint32_t)p;
    deltas[s][at] = delta;
  }
  // the head of rank `at` is the begin event at and closes the interval at - 1: segment and end of the maximum in front of it
  __device__ __forceinline__ void head(int s, uint32_t at, uint64_t key, unsigned long long prev) const {
    event(s, at, key, 1u);
    if (at > 0) event(s, (uint64_t)total[s] + at - 1, prev, ~0u);
  }
  __device__ __forceinline__ void last(int s, unsigned long long max_p) const { event(s, 2 * (uint64_t)total[s] - 1, max_p, ~0u); }
};

__global__ __launch_bounds__(TB) void sharing_count_kernel(uint64_t n2, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry,
                                                           uint64_t ntiles, SegMap M, uint32_t sets, uint32_t* __restrict__ tile_cnt) {
  heads_tile<false>(n2, keys, vals, ends, carry, ntiles, M.sentinel, sets, tile_cnt, EventsOut{});
}

__global__ __launch_bounds__(TB) void sharing_events_kernel(uint64_t n2, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ carry,
                                                            uint64_t ntiles, uint32_t sets, uint32_t* __restrict__ tile_off, EventsOut out) {
  heads_tile<true>(n2, keys, vals, ends, carry, ntiles, out.M.sentinel, sets, tile_off, out);
}

// ---- the depth sweep over the sorted events of one set ---------------------------------------------------------------------
__global__ __launch_bounds__(TB) void sharing_group_first_kernel(const uint64_t* __restrict__ keys, uint64_t n_ev, uint32_t* __restrict__ first) {
  const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (p >= n_ev) return;
  first[p] = p > 0 && keys[p - 1] != keys[p] ? (uint32_t)p : 0u;  // (event 0 begins a group at 0)
}

// before[p]: the exclusive scan of the deltas; first[p]: where p's group begins
__global__ __launch_bounds__(TB) void sharing_break_flags_kernel(const uint64_t* __restrict__ keys, uint64_t n_ev, const uint32_t* __restrict__ before,
                                                                 const uint32_t* __restrict__ first, uint8_t* __restrict__ flag) {
  const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (p >= n_ev) return;
  const bool last = p + 1 == n_ev || keys[p + 1] != keys[p];
  const uint32_t behind = p + 1 == n_ev ? 0u : before[p + 1];  // (all deltas cancel)
  flag[p] = last && behind != before[first[p]];
}

__global__ __launch_bounds__(TB) void sharing_open_flags_kernel(const uint32_t* __restrict__ breaks, uint64_t n_breaks, const uint64_t* __restrict__ keys,
                                                                uint64_t n_ev, const uint32_t* __restrict__ before, uint64_t* __restrict__ b_key,
                                                                uint32_t* __restrict__ b_depth, uint8_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_breaks) return;
  const uint64_t p = breaks[i];
  const uint32_t depth = p + 1 >= n_ev ? 0u : before[p + 1];
  b_key[i] = keys[p];
  b_depth[i] = depth;
  flag[i] = depth != 0;
}

__global__ __launch_bounds__(TB) void sharing_runs_kernel(const uint32_t* __restrict__ openers, uint64_t n_runs, const uint64_t* __restrict__ b_key,
                                                          const uint32_t* __restrict__ b_depth, uint64_t n_breaks, swg_depth_run* __restrict__ rows) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= n_runs) return;
  const uint64_t i = openers[j];
  const uint64_t key = b_key[i];
  // (always i + 1 < n_breaks: the depth is 0 behind a sequence's last event, so an opener is never the last breakpoint)
  const uint32_t end = i + 1 < n_breaks ? (uint32_t)b_key[i + 1] : (uint32_t)key;
  rows[j] = swg_depth_run{(uint32_t)(key >> 32), (uint32_t)key, end, b_depth[i]};
}

__global__ __launch_bounds__(TB) void sharing_bases_kernel(const swg_depth_run* __restrict__ rows, uint64_t n_rows, unsigned long long* __restrict__ sum) {
  bases_sum(rows, n_rows, sum);
}

// `amount` of every lane with a key (EMPTY = none) into the spectrum: runs of one key along the lanes are summed towards their
// first lane, which goes through the work-group's table.  Called by whole wavefronts.
__device__ __forceinline__ void spectrum_add(LdsTable<1, false>& lds, const Spectrum& T, unsigned long long key, unsigned long long amount) {
  const int lane = threadIdx.x & 63;
  unsigned long long v[1] = {amount};
  const unsigned long long left = __shfl_up(key, 1);
  const bool first_lane = lane == 0 || key != left;
  const int end = run_end(__ballot(first_lane), lane);
  run_sum(v, lane, end);
  if (first_lane && key != EMPTY && v[0]) {
    if (!lds.add(key, v)) table_add<1, false>(T, key, v, 0);  // more keys in this work-group's share than the LDS table takes
  }
}

__global__ __launch_bounds__(TB) void sharing_spectrum_kernel(const swg_depth_run* __restrict__ rows, uint64_t n_rows, const uint32_t* __restrict__ seq_genome,
                                                              uint32_t G, Spectrum T) {
  __shared__ LdsTable<1, false> l_table;
  l_table.clear();
  __syncthreads();
  for (uint64_t base = (uint64_t)blockIdx.x * TB; base < n_rows; base += (uint64_t)gridDim.x * TB) {  // (uniform: whole wavefronts vote)
    const uint64_t x = base + threadIdx.x;
    unsigned long long key = EMPTY, amount = 0;
    if (x < n_rows) {
      const swg_depth_run r = rows[x];
      if (r.depth < G) key = (unsigned long long)seq_genome[r.seq] * G + r.depth, amount = r.end - r.start;  // (always: depth <= G - 1)
    }
    spectrum_add(l_table, T, key, amount);
  }
  __syncthreads();
  l_table.flush(T, 0);
}

__global__ __launch_bounds__(TB) void sharing_lengths_kernel(const uint32_t* __restrict__ seq_len, const uint32_t* __restrict__ seq_genome, uint32_t n_seq,
                                                             uint32_t G, Spectrum T, unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<1, false> l_table;
  l_table.clear();
  __syncthreads();
  for (uint64_t base = (uint64_t)blockIdx.x * TB; base < n_seq; base += (uint64_t)gridDim.x * TB) {
    const uint64_t s = base + threadIdx.x;
    unsigned long long key = EMPTY, amount = 0;
    if (s < n_seq) {
      const uint32_t g = seq_genome[s];
      if (g < G) key = (unsigned long long)g * G, amount = seq_len[s];
      else atomicOr(&scalars[D_BAD], 1ull);
    }
    spectrum_add(l_table, T, key, amount);
  }
  __syncthreads();
  l_table.flush(T, 0);
}

// one work-group per genome: column 0 holds the genome's length, the other entries of the row are taken off it
__global__ __launch_bounds__(TB) void sharing_private_kernel(unsigned long long* __restrict__ spectrum, uint32_t G) {
  __shared__ unsigned long long l_sum[WAVES];
  unsigned long long* row = spectrum + (uint64_t)blockIdx.x * G;
  unsigned long long s = 0;
  for (uint32_t d = 1 + threadIdx.x; d < G; d += TB) s += row[d];
  const unsigned long long t = block_sum(s, l_sum);
  if (threadIdx.x == 0) row[0] -= t;
}

// The depth sweep of one set over its 2 m events (unsorted in ev_keys / ev_deltas), inside an arena frame: the runs on the
// device, then what `runs` (n, bases, rows) and `spectrum` ask for.  vec: receives the rows instead of list->rows.
int depth_sweep(swg_ctx* ctx, uint32_t m, uint64_t* ev_keys, uint32_t* ev_deltas, uint32_t n_seq, uint32_t G, const SegCols& d, bool runs, bool spectrum,
                unsigned long long* scalars, unsigned long long* sc, swg_depth_list* list, std::vector<swg_depth_run>* vec) {
  hipStream_t st = ctx->stream;
  const uint64_t n_ev = 2 * (uint64_t)m;
  uint64_t n_breaks = 0, n_runs = 0;
  swg_depth_run* rows = nullptr;
  if (m) {
    uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n_ev);
    uint32_t* deltas_alt = swg_alloc<uint32_t>(ctx, n_ev);
    uint32_t* first = swg_alloc<uint32_t>(ctx, n_ev);
    uint8_t* flag = swg_alloc<uint8_t>(ctx, n_ev);
    SWG_CHECK_ARENA(ctx);
    {
      swg_prof_scope sort_scope(ctx, "sharing_sort_events");
      SWG_TRY(swg_radix_sort_pairs(ctx, &ev_keys, &ev_deltas, &keys_alt, &deltas_alt, n_ev, 0, 32 + swg_bits_for(n_seq)));
    }
    uint32_t* before = deltas_alt;  // (the sort is over: whichever buffer it left free)
    SWG_TRY(swg_exclusive_scan_u32(ctx, ev_deltas, before, n_ev, nullptr));
    const unsigned grid_e = (unsigned)((n_ev + TB - 1) / TB);
    SWG_LAUNCH(ctx, "sharing_group_first", sharing_group_first_kernel<<<grid_e, TB, 0, st>>>(ev_keys, n_ev, first));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_inclusive_max_scan_u32(ctx, first, first, n_ev));
    SWG_LAUNCH(ctx, "sharing_break_flags", sharing_break_flags_kernel<<<grid_e, TB, 0, st>>>(ev_keys, n_ev, before, first, flag));
    SWG_KERNEL_CHECK(ctx);
    swg_flag_scan fs{};
    SWG_TRY(swg_flags_count(ctx, flag, n_ev, &fs, reinterpret_cast<uint64_t*>(sc + S_BREAKS)));
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(sc + S_BREAKS), &n_breaks, 1));
    if (n_breaks) {  // (always: the first event of the first sequence raises the depth from 0)
      uint32_t* breaks = swg_alloc<uint32_t>(ctx, n_breaks);
      uint64_t* b_key = swg_alloc<uint64_t>(ctx, n_breaks);
      uint32_t* b_depth = swg_alloc<uint32_t>(ctx, n_breaks);
      uint8_t* b_flag = swg_alloc<uint8_t>(ctx, n_breaks);
      SWG_CHECK_ARENA(ctx);
      SWG_TRY(swg_flags_compact(ctx, fs, breaks));
      const unsigned grid_b = (unsigned)((n_breaks + TB - 1) / TB);
      SWG_LAUNCH(ctx, "sharing_open_flags", sharing_open_flags_kernel<<<grid_b, TB, 0, st>>>(breaks, n_breaks, ev_keys, n_ev, before, b_key, b_depth, b_flag));
      SWG_KERNEL_CHECK(ctx);
      swg_flag_scan fo{};
      SWG_TRY(swg_flags_count(ctx, b_flag, n_breaks, &fo, reinterpret_cast<uint64_t*>(sc + S_RUNS)));
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(sc + S_RUNS), &n_runs, 1));
      if (n_runs) {
        uint32_t* openers = swg_alloc<uint32_t>(ctx, n_runs);
        rows = swg_alloc<swg_depth_run>(ctx, n_runs);
        SWG_CHECK_ARENA(ctx);
        SWG_TRY(swg_flags_compact(ctx, fo, openers));
        SWG_LAUNCH(ctx, "sharing_runs", sharing_runs_kernel<<<(unsigned)((n_runs + TB - 1) / TB), TB, 0, st>>>(openers, n_runs, b_key, b_depth, n_breaks, rows));
        SWG_KERNEL_CHECK(ctx);
      }
    }
  }
  if (runs) {
    uint64_t bases = 0;
    if (n_runs) {
      SWG_LAUNCH(ctx, "sharing_bases", sharing_bases_kernel<<<grid_for(ctx, n_runs), TB, 0, st>>>(rows, n_runs, sc + S_BASES));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(sc + S_BASES), &bases, 1));
    }
    list->n = n_runs;
    list->bases = bases;
    swg_depth_run* dst;
    SWG_TRY(rows_hand_over(ctx, rows, n_runs, vec, list->rows, list->capacity, &dst));
  }
  if (spectrum) {
    Spectrum T{};
    T.slots = (uint64_t)G * G;
    T.sums = swg_alloc<unsigned long long>(ctx, T.slots);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(T.sums, 0, T.slots * sizeof(unsigned long long), st));
    if (n_runs) {
      SWG_LAUNCH(ctx, "sharing_spectrum", sharing_spectrum_kernel<<<grid_for(ctx, n_runs), TB, 0, st>>>(rows, n_runs, d.seq_genome, G, T));
      SWG_KERNEL_CHECK(ctx);
    }
    if (d.seq_len) {
      SWG_LAUNCH(ctx, "sharing_lengths", sharing_lengths_kernel<<<grid_for(ctx, n_seq), TB, 0, st>>>(d.seq_len, d.seq_genome, n_seq, G, T, scalars));
      SWG_KERNEL_CHECK(ctx);
      SWG_LAUNCH(ctx, "sharing_private", sharing_private_kernel<<<G, TB, 0, st>>>(T.sums, G));
      SWG_KERNEL_CHECK(ctx);
      uint64_t bad = 0;
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + D_BAD), &bad, 1));
      if (bad & 1u) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: a genome id >= n_genome in seq_genome");
    }
    SWG_HIP(ctx, hipMemcpyAsync(list->spectrum, T.sums, T.slots * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SWG_HIP(ctx, hipStreamSynchronize(st));
  }
  return SWG_OK;
}

// inside an arena frame.  vecs: nullptr, or [2] vectors that receive the rows instead of req's arrays
int sharing_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, uint32_t G, const SegCols& d, swg_sharing_request* req, std::vector<swg_depth_run>* vecs) {
  hipStream_t st = ctx->stream;
  const uint32_t want = req->want;
  const uint32_t sets = (want & 0x5u ? SET_ALL : 0u) | (want & 0xau ? SET_KEPT : 0u);
  const uint64_t n2 = 2 * n, ntiles = (n2 + TILE - 1) / TILE;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  EventsOut out{};
  if (n) {
    uint64_t* keys = swg_alloc<uint64_t>(ctx, n2);
    uint64_t* keys_alt = swg_alloc<uint64_t>(ctx, n2);
    uint32_t* vals = swg_alloc<uint32_t>(ctx, n2);
    uint32_t* vals_alt = swg_alloc<uint32_t>(ctx, n2);
    uint32_t* ends = swg_alloc<uint32_t>(ctx, n2);
    unsigned long long* tile_max = swg_alloc<unsigned long long>(ctx, 2 * ntiles);
    uint32_t* tile_cnt = swg_alloc<uint32_t>(ctx, 2 * ntiles);
    SegMap M;
    segmap_alloc(ctx, n2, n_seq, G, segmap_forced(), &M);  // (every record may touch two segments)
    SWG_CHECK_ARENA(ctx);
    out.M = M;
    if (M.set_keys) SWG_HIP(ctx, hipMemsetAsync(M.set_keys, 0xff, ((size_t)M.set_mask + 1) * sizeof(unsigned long long), st));
    const unsigned grid_n = (unsigned)((n + TB - 1) / TB), grid_t = (unsigned)ntiles;
    SWG_LAUNCH(ctx, "sharing_keys", sharing_keys_kernel<<<grid_n, TB, 0, st>>>(n, d.q_id, d.t_id, d.start[0], d.start[1], d.end[0], d.end[1], d.status,
                                                                               d.seq_genome, d.seq_len, n_seq, M, keys, vals, scalars));
    SWG_KERNEL_CHECK(ctx);
    {
      swg_prof_scope sort_scope(ctx, "sharing_sort");
      SWG_TRY(swg_radix_sort_pairs(ctx, &keys, &vals, &keys_alt, &vals_alt, n2, 0, 32 + swg_bits_for(M.sentinel)));
    }
    SWG_LAUNCH(ctx, "sharing_gather", sharing_gather_kernel<<<grid_t, TB, 0, st>>>(n2, keys, vals, d.end[0], d.end[1], M.sentinel, ends, tile_max, ntiles));
    SWG_KERNEL_CHECK(ctx);
    for (int s = 0; s < 2; ++s)
      if (sets >> s & 1u)
        SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max + s * ntiles), reinterpret_cast<uint64_t*>(tile_max + s * ntiles), ntiles));
    SWG_LAUNCH(ctx, "sharing_count", sharing_count_kernel<<<grid_t, TB, 0, st>>>(n2, keys, vals, ends, tile_max, ntiles, M, sets, tile_cnt));
    SWG_KERNEL_CHECK(ctx);
    for (int s = 0; s < 2; ++s)
      if (sets >> s & 1u)
        SWG_TRY(swg_exclusive_scan_u32(ctx, tile_cnt + s * ntiles, tile_cnt + s * ntiles, ntiles, reinterpret_cast<uint64_t*>(scalars + D_HEADS + s)));
    uint64_t h[D_SET];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_SET));
    if (h[D_BAD] & 1u) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: a sequence id >= n_seq or a genome id >= n_genome");
    if (h[D_BAD] & 2u) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: a record ends beyond seq_len of its sequence");
    for (int s = 0; s < 2; ++s) {
      if (!(sets >> s & 1u)) continue;
      out.total[s] = (uint32_t)h[D_HEADS + s];  // (<= 2 n < 2^31)
      out.keys[s] = swg_alloc<uint64_t>(ctx, 2 * (uint64_t)out.total[s] + 1);
      out.deltas[s] = swg_alloc<uint32_t>(ctx, 2 * (uint64_t)out.total[s] + 1);
    }
    SWG_CHECK_ARENA(ctx);
    if (out.total[0] || out.total[1]) {
      SWG_LAUNCH(ctx, "sharing_events", sharing_events_kernel<<<grid_t, TB, 0, st>>>(n2, keys, vals, ends, tile_max, ntiles, sets, tile_cnt, out));
      SWG_KERNEL_CHECK(ctx);
    }
  }
  for (int s = 0; s < 2; ++s) {
    if (!(sets >> s & 1u)) continue;
    const swg_arena_mark mark = swg_arena_save(ctx);  // (a set's sweep goes back to the arena behind it)
    SWG_TRY(depth_sweep(ctx, out.total[s], out.keys[s], out.deltas[s], n_seq, G, d, (want >> s & 1u) != 0, (want >> (2 + s) & 1u) != 0, scalars,
                        scalars + D_SET + s * S_COUNT, &req->set[s], vecs ? &vecs[s] : nullptr));
    swg_arena_restore(ctx, mark);
  }
  return SWG_OK;
}

// the seams' argument checks, then the device work inside an arena frame
int sharing_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint32_t* seq_len,
                const uint8_t* status, swg_sharing_request* req, std::vector<swg_depth_run>* vecs) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: NULL records or request");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: reserved must be 0");
  const uint32_t want = req->want;
  if (want == 0 || want >> 4) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: want names nothing, or a bit beyond the four");
  if (!status && (want & 0xau)) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: the KEPT runs and spectrum need a status column");
  for (int s = 0; s < 2; ++s)
    if ((want >> (2 + s) & 1u) && !req->set[s].spectrum) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: a spectrum bit with a NULL spectrum");
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  SWG_TRY(seg_check_args(ctx, "sharing", ARG_LIMIT, rec, seq_genome, n_genome, 30));
  if ((want & WANT_SPECTRUM) && n_genome > MAX_SPECTRUM_GENOMES)
    return swg_set_error(ctx, SWG_ERR_RANGE, "sharing: a spectrum of more than 4096 genomes (the runs alone have no such limit)");
  for (int s = 0; s < 2; ++s) {
    if (want >> s & 1u) {
      req->set[s].n = req->set[s].bases = 0;
      if (vecs) vecs[s].clear();
    }
    if (want >> (2 + s) & 1u) std::memset(req->set[s].spectrum, 0, (size_t)n_genome * n_genome * sizeof(uint64_t));
  }
  const bool lengths = (want & WANT_SPECTRUM) && seq_len && n_seq;  // (column 0 needs the device even without records)
  if (n == 0 && !lengths) return SWG_OK;
  if (n && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end))
    return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: NULL column (q_id, t_id and the four coordinates are read)");
  if (!seq_genome) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: NULL seq_genome");
  SWG_TRY(seg_check_args(ctx, "sharing", ARG_COUNTS, rec, seq_genome, n_genome, 30));
  if (n == 0 && !on_device) {  // no record, nothing to sweep: column 0 is the lengths, and they are here
    for (int s = 0; s < 2; ++s) {
      if (!(want >> (2 + s) & 1u)) continue;
      for (uint32_t q = 0; q < n_seq; ++q) {
        if (seq_genome[q] >= n_genome) return swg_set_error(ctx, SWG_ERR_INVALID, "sharing: a genome id >= n_genome in seq_genome");
        req->set[s].spectrum[(size_t)seq_genome[q] * n_genome] += seq_len[q];
      }
    }
    return SWG_OK;
  }
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * 96 + (size_t)n_seq * 8 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    SegCols d;
    SWG_TRY(seg_stage(ctx, rec, on_device, seq_genome, status, &d));
    d.seq_len = seq_len;
    if (!on_device) {
      swg_stager s(ctx);
      s.add(&d.seq_len, n_seq);
      SWG_TRY(s.run());
    }
    return sharing_device(ctx, n, n_seq, n_genome, d, req, vecs);
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint32_t* seq_len,
                const uint8_t* status, swg_sharing_request* req) {
  try {
    return sharing_run(ctx, rec, on_device, seq_genome, n_genome, seq_len, status, req, nullptr);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

// the table of swg_paf_sharing from the two spectra ([G * G] each)
std::string table_text(const std::vector<std::string>& gname, const std::vector<uint64_t> (&spectrum)[2], bool detailed) {
  std::string o = "genome\tlength\tprivate_all\tshared_all\tcore_all\tprivate_kept\tshared_kept\tcore_kept\n";
  const size_t G = gname.size();
  if (!G) return o;
  uint64_t total[7] = {0, 0, 0, 0, 0, 0, 0};
  for (size_t g = 0; g < G; ++g) {
    uint64_t row[7] = {0, 0, 0, 0, 0, 0, 0};  // length, then private / shared / core of ALL and of KEPT
    for (int s = 0; s < 2; ++s)
      for (size_t d = 0; d < G; ++d) {
        const uint64_t v = spectrum[s][g * G + d];
        if (s == 0) row[0] += v;
        row[1 + 3 * s + (d == 0 ? 0 : d == G - 1 ? 2 : 1)] += v;
      }
    o += gname[g];
    o += '\t';
    for (int c = 0; c < 7; ++c) {
      append_u64(o, row[c], c == 6 ? '\n' : '\t');
      total[c] += row[c];
    }
  }
  o += "#total\t";
  for (int c = 0; c < 7; ++c) append_u64(o, total[c], c == 6 ? '\n' : '\t');
  if (detailed) {
    o += "#spectrum\n";
    for (size_t g = 0; g < G; ++g)
      for (int s = 0; s < 2; ++s)
        for (size_t d = 0; d < G; ++d) {
          const uint64_t v = spectrum[s][g * G + d];
          if (!v) continue;
          o += gname[g];
          o += s ? "\tkept\t" : "\tall\t";
          append_u64(o, d, '\t');
          append_u64(o, v, '\n');
        }
  }
  return o;
}

// the BED of swg_paf_sharing: the joint runs of the two sorted lists.  Every KEPT run lies under ALL runs (a kept record is a
// record), so the pieces are the ALL runs cut at the KEPT runs' borders.
std::string bed_text(const swg_paf* p, const std::vector<swg_depth_run>& all, const std::vector<swg_depth_run>& kept) {
  std::string o;
  swg_depth_run open{0, 0, 0, 0};  // the piece being grown; open.depth = n_all, open_kept = n_kept
  uint32_t open_kept = 0;
  bool have = false;
  auto flush = [&]() {
    if (!have) return;
    o += swg_paf_sequence_name(p, open.seq);
    o += '\t';
    append_u64(o, open.start, '\t');
    append_u64(o, open.end, '\t');
    append_u64(o, open.depth, '\t');
    append_u64(o, open_kept, '\n');
  };
  auto piece = [&](uint32_t seq, uint32_t from, uint32_t to, uint32_t n_all, uint32_t n_kept) {
    if (from >= to) return;
    if (have && open.seq == seq && open.end == from && open.depth == n_all && open_kept == n_kept) {
      open.end = to;
      return;
    }
    flush();
    open = swg_depth_run{seq, from, to, n_all};
    open_kept = n_kept;
    have = true;
  };
  size_t j = 0;
  for (const swg_depth_run& a : all) {
    while (j < kept.size() && (kept[j].seq < a.seq || (kept[j].seq == a.seq && kept[j].end <= a.start))) ++j;
    uint32_t at = a.start;
    for (size_t x = j; x < kept.size() && kept[x].seq == a.seq && kept[x].start < a.end; ++x) {
      const uint32_t from = std::max(kept[x].start, a.start), to = std::min(kept[x].end, a.end);
      piece(a.seq, at, from, a.depth, 0);
      piece(a.seq, from, to, a.depth, kept[x].depth);
      at = to;
    }
    piece(a.seq, at, a.end, a.depth, 0);
  }
  flush();
  return o;
}

}  // namespace

extern "C" int swg_sharing_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint32_t* seq_len,
                                   const uint8_t* status, swg_sharing_request* req) {
  return records_abi(ctx, rec, false, seq_genome, n_genome, seq_len, status, req);
}

extern "C" int swg_sharing_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome,
                                          const uint32_t* seq_len, const uint8_t* status, swg_sharing_request* req) {
  return records_abi(ctx, rec, true, seq_genome, n_genome, seq_len, status, req);
}

// The sharing texts of an open PAF: records and genome map from the handle (the last-'#' map of swg_paf_breadth), seq_len from
// the handle's text (swg_paf_components' rule), runs and spectra of both sets from ONE device call, names from the handle.
// Errors: swg_alnstats_last_error().
extern "C" int swg_paf_sharing(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, int detailed, char* out_text[2], uint64_t out_len[2]) {
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_sharing: NULL argument");
  const bool wanted[2] = {out_text[0] != nullptr, out_text[1] != nullptr};
  out_text[0] = out_text[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_sharing: neither text is asked for");
  if (!status) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_sharing: the kept columns need a status column");
  const uint64_t n = swg_paf_records(p)->n;
  if (n && !ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_sharing: NULL context");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "swg_paf_sharing: the file has a value >= 2^32, its columns are rebased: sharing of 64-bit columns is not supported");
  try {
    std::vector<swg_depth_run> rows[2];
    std::vector<uint64_t> spectrum[2];
    std::vector<std::string> gname;
    if (n) {
      swg_records rec;
      std::vector<uint32_t> col10, seq_len;
      const uint32_t* seq_genome = nullptr;
      SWG_TRY(swg_paf_stats_prepare(p, &rec, &col10, &seq_genome));
      SWG_TRY(swg_paf_seq_last_lengths(p, &seq_len));
      const uint32_t G = rec.n_genome_last;
      swg_sharing_request req{};
      if (wanted[0]) {
        if (G > MAX_SPECTRUM_GENOMES) return swg_alnstats_error(SWG_ERR_RANGE, "swg_paf_sharing: the table takes at most 4096 genomes");
        req.want |= WANT_SPECTRUM;
        for (int s = 0; s < 2; ++s) {
          spectrum[s].assign((size_t)G * G, 0);
          req.set[s].spectrum = spectrum[s].data();
        }
      }
      if (wanted[1]) req.want |= WANT_RUNS;
      const int rc = sharing_run(ctx, &rec, false, seq_genome, G, seq_len.data(), status, &req, rows);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
      swg_paf_stats_genome_names(p, &gname);
    }
    const std::string text[2] = {wanted[0] ? table_text(gname, spectrum, detailed != 0) : std::string(),
                                 wanted[1] ? bed_text(p, rows[0], rows[1]) : std::string()};
    return texts_hand_over(text, wanted, 2, out_text, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
