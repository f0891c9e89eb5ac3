// What the lift (swg_lift.hip) and the transitive lift (swg_lift_closure.hip, section 24) share: the per-axis
// index over the records -- built once, joined as often as the caller likes -- and the device side of a join: the binary searches
// that give a region its candidate range, and the expansion of a tile's region heads in LDS.
#pragma once
#include "swg_internal.h"
#include "swg_pair_table.h"

namespace swg_lift_ix {

using swg_pair_table::TB;
using swg_pair_table::WAVES;
// device scalars of lift_limits: bad input (bit 0: a record id out of range; bits 1-3 are the regions': reserved != 0, start > end,
// a seq neither < n_seq nor UINT32_MAX), the largest start of a record of non-zero length per axis
enum { D_BAD = 0, D_MAX_START = 1 };
constexpr int T = 1024;        // candidates per tile
constexpr int ITEMS = T / TB;  // per thread
constexpr uint32_t KEPT_BIT = 0x80000000u;
constexpr uint32_t UNKNOWN_SEQ = 0xffffffffu;

struct LiftCols {
  const uint32_t *id[2], *start[2], *end[2];  // [axis]: 0 = query, 1 = target
  const uint8_t *strand, *status;
};

// One axis' index, in the arena frame of the call that built it: the records of non-zero length in (sequence, start, record) order.
struct LiftIndex {
  uint64_t* keys = nullptr;  // [n] seq << pb | start; records of zero length carry the sentinel sequence n_seq
  uint64_t* M = nullptr;     // [n] running maximum of seq << 32 | end: a per-sequence prefix maximum of the ends
  uint32_t* V = nullptr;     // [n] record | KEPT_BIT
  uint32_t* E = nullptr;     // [n] the record's end
  uint64_t max_start = 0;
  int pb = 0;
};

// lift_limits over the records: scalars[D_BAD] bit 0 and scalars[D_MAX_START + axis] (device words, zero before)
int swg_lift_limits(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, unsigned long long* scalars);
// lift_keys, the radix sort, lift_gather and the prefix maximum for one axis: 24 bytes of arena per record
int swg_lift_index_build(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, uint32_t axis, uint64_t max_start, LiftIndex* out);

// The lift's own seams for the calls built on it (the exact lift and the hit records, swg_cigar.hip).
// The checks of swg_lift_records on the request (set, axes, status, regions, the two ranges) and, once there is device work, on the
// columns and the host regions: the same errors in the same words.
int swg_lift_check_request(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m, uint32_t set,
                           uint32_t axes);
int swg_lift_check_columns(swg_ctx* ctx, const swg_records* rec, bool on_device, const swg_lift_region* regions, uint64_t m);
// the host columns of c (strand and status with them) and the regions into the stager, in the order swg_lift_records stages them
void swg_lift_stage(swg_stager* s, uint64_t n, uint64_t m, LiftCols* c, const swg_lift_region** regions);
// The whole lift inside the caller's arena frame (c and regions: device pointers): req's n, candidates and summary as
// swg_lift_records fills them, but the finished rows stay in the frame -- dev->rows, NULL when there are none or they were not
// written -- and req->rows is only looked at as "rows are wanted" (with req->capacity) unless `always` is set.
struct LiftDeviceRows {
  bool always = false;
  const swg_lift_row* rows = nullptr;
};
int swg_lift_rows_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const LiftCols& c, const swg_lift_region* regions, uint64_t m,
                         swg_lift_request* req, LiftDeviceRows* dev);

#ifdef __HIPCC__
// the first position of a[0 .. n) whose value is >= v (n when none)
__device__ __forceinline__ uint64_t lower_bound64(const uint64_t* __restrict__ a, uint64_t n, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the first region whose scanned offset exceeds v: the region that candidate v of the stream belongs to
__device__ __forceinline__ uint64_t region_of(const uint64_t* __restrict__ W, uint64_t m, uint64_t v) { return lower_bound64(W, m, v + 1); }

// The candidates of the non-empty region [a, b) of sequence seq < n_seq: hi = the first position with start >= b, p0 = the first
// position of the sequence whose prefix maximum of ends exceeds a.  Every hit lies in [p0, hi); returns hi - p0.
__device__ __forceinline__ uint64_t lift_candidates(uint64_t n, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ M, int pb,
                                                    uint64_t max_start, uint32_t seq, uint32_t a, uint32_t b, uint32_t* p0) {
  const uint64_t base = (uint64_t)seq << pb;
  const uint64_t lo = lower_bound64(keys, n, base);
  const uint64_t cut = b < max_start + 1 ? b : max_start + 1;  // (base + max_start + 1 may be the next sequence's first key: right)
  const uint64_t hi = lo + lower_bound64(keys + lo, n - lo, base + cut);
  // inside [lo, hi) the high half of M is seq: M > seq << 32 | a  <=>  the prefix maximum of the ends exceeds a
  const uint64_t at = lo + lower_bound64(M + lo, hi - lo, (((uint64_t)seq << 32) | a) + 1);
  *p0 = (uint32_t)at;
  return hi - at;
}

// The heads of one tile of the candidate stream, by the whole work-group: candidates [g0, g0 + cnt) of the stream whose scanned
// widths are W[0 .. m).  Afterwards l_hs[slot] is the slot where the slot's region begins in this tile, and at such a head slot h:
// l_hreg[h] the region, l_ha[h] its start, l_hbase[h] = (p0 - h) mod 2^32, so that the index position of a slot is l_hbase[h] +
// slot.  Regions without candidates are walked over, never expanded.  All LDS arrays hold T words but l_wave (WAVES) and l_span (2).
// Ends with a barrier; the caller may zero LDS of its own before the call (the first barrier inside covers it).
__device__ __forceinline__ void lift_tile_heads(const uint64_t* __restrict__ W, uint64_t m, const uint32_t* __restrict__ first,
                                                const swg_lift_region* __restrict__ regions, uint64_t g0, uint32_t cnt, uint32_t* l_hs,
                                                uint32_t* l_hreg, uint32_t* l_ha, uint32_t* l_hbase, uint32_t* l_wave, uint64_t* l_span) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) l_span[0] = region_of(W, m, g0);
  if (threadIdx.x == 64) l_span[1] = region_of(W, m, g0 + cnt - 1);
  for (int s = threadIdx.x; s < T; s += TB) l_hs[s] = 0;
  __syncthreads();
  const uint64_t rf = l_span[0], rl = l_span[1];  // (rf <= rl < m: both candidates exist)
  if (threadIdx.x == 0) {
    const uint64_t before = rf ? W[rf - 1] : 0;
    l_hreg[0] = (uint32_t)rf;
    l_ha[0] = regions[rf].start;
    l_hbase[0] = first[rf] + (uint32_t)(g0 - before);
  }
  for (uint64_t r = rf + 1 + threadIdx.x; r <= rl; r += TB) {  // regions that begin inside the tile; those without candidates fall through
    const uint64_t before = W[r - 1];
    if (W[r] == before) continue;
    const uint32_t s = (uint32_t)(before - g0);
    if (s >= (uint32_t)T) continue;  // (never)
    l_hs[s] = s;
    l_hreg[s] = (uint32_t)r;
    l_ha[s] = regions[r].start;
    l_hbase[s] = first[r] - s;
  }
  __syncthreads();
  {  // running maximum of the head slots: blocked, ITEMS slots per thread
    uint32_t h[ITEMS], run = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      h[j] = l_hs[threadIdx.x * ITEMS + j];
      run = h[j] > run ? h[j] : run;
      h[j] = run;
    }
    uint32_t inc = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= d && o > inc) inc = o;
    }
    if (lane == 63) l_wave[wave] = inc;
    __syncthreads();
    uint32_t carry = __shfl_up(inc, 1);
    if (lane == 0) carry = 0;
    for (int w = 0; w < wave; ++w) carry = l_wave[w] > carry ? l_wave[w] : carry;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) l_hs[threadIdx.x * ITEMS + j] = h[j] > carry ? h[j] : carry;
  }
  __syncthreads();
}
#endif

}  // namespace swg_lift_ix
