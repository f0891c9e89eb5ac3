// Lift slices: every exact row of the lift as an alignment of its own -- its four coordinates, block length
// and the CIGAR text cut at its first and last aligned column.  The rows are swg_lift.hip's, the parse, the four prefix sums,
// chunk_rank[] and the entry states are cigar_build's (swg_cigar.hip, swg_cigar_build.h); include/sweepga_gpu.h states the
// definitions, swg_slice_walk.h holds the rules.
//
//   slice_op_pos  one thread per 16 text bytes, one load: the chunk's ops are ranked from chunk_rank[] and each writes the position of
//                 its letter, relative to its entry's first byte (the entry by binary search in offset[], once per chunk and again only
//                 where a chunk holds an entry border).
//   slice_rows    one thread per row of the lift: the record's entry by binary search, and on state 0 the slice and its copy plan
//                 (slice_of: four searches in the record's prefix sums); a keep flag; the rows without a slice are counted per
//                 wavefront.
//   (compaction)  swg_flags_count / swg_flags_compact: the kept rows, ascending; their number is read back.
//   slice_gather  one thread per slice: slice and plan to their place, text_len into the scan's array.
//   (scan)        swg_inclusive_sum_scan_u64 over the text lengths: where each slice's text ends, and the text's length (read back).
//   slice_first   one thread per slice: text_first.
//   slice_text    the output text in tiles of SWG_SLICE_TEXT_TILE bytes, one work-group each: two searches in the ends give the
//                 slices the tile touches, their ends go to LDS, and every output byte finds its slice there and its value from the
//                 slice's plan (text_byte): head digits, verbatim bytes and tail digits are all addressed from the output position, so
//                 a slice of megabytes and thousands of slices of nine bytes load the lanes alike.  W output bytes per lane and store:
//                 1, or 4 packed into one dword.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "swg_internal.h"
#include "swg_lift_index.h"
#include "swg_pair_table.h"
#include "swg_cigar_build.h"
#include "swg_slice_walk.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;  // TB, WAVES, reserve_first
using namespace swg_lift_ix;
using namespace swg_cigar;
using namespace swg_slice;

constexpr int TILE = (int)SWG_SLICE_TEXT_TILE;
constexpr int MAX_SLOTS = TILE / 2 + 2;  // a slice's text has two bytes or more: at most TILE / 2 + 1 slices touch a tile
static_assert(TB == 256 && WAVES == 4 && TILE % (4 * TB) == 0, "whole rounds of the work-group per tile, in either form");
static_assert(sizeof(swg_lift_slice) == 56 && sizeof(swg_lift_slice_request) == 120 && sizeof(swg_lift_paf_counts) == 64 && sizeof(Plan) == 24,
              "include/sweepga_gpu.h states these sizes");
enum { L_INTERP = C_BUILD_TOTAL, L_EMPTY, L_SHORT, L_SLICES, L_LONG, L_TOTAL };

unsigned grid_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

__device__ __forceinline__ void count_votes(bool vote, unsigned long long* slot) {
  const uint64_t votes = __ballot(vote);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(slot, (unsigned long long)__popcll(votes));
}

// the last entry j in [lo, hi] with offset[j] <= pos (offset[lo] <= pos)
__device__ __forceinline__ uint64_t entry_at(const uint64_t* __restrict__ offset, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo + 1) >> 1);
    if (offset[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(TB) void slice_op_pos_kernel(CigarSet S, int aligned, uint32_t* __restrict__ pos) {
  const uint64_t chunk = (uint64_t)blockIdx.x * TB + threadIdx.x, p0 = chunk * 16;
  if (p0 >= S.B) return;
  const uint32_t n = S.B - p0 < 16 ? (uint32_t)(S.B - p0) : 16u;
  unsigned char b[16];
  if (aligned && n == 16) {
    *reinterpret_cast<uint4*>(b) = *reinterpret_cast<const uint4*>(S.text + p0);
  } else {
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) b[q] = q < n ? (unsigned char)S.text[p0 + q] : (unsigned char)'0';
  }
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t q = 0; q < 16; ++q) mask |= (is_digit(b[q]) ? 0u : 1u) << q;
  if (!mask) return;
  uint32_t rank = S.chunk_rank[chunk];
  const uint64_t j_lo = entry_at(S.offset, 0, S.k - 1, p0), j_hi = entry_at(S.offset, j_lo, S.k - 1, p0 + n - 1);
  while (mask) {
    const int q = __builtin_ctz(mask);
    mask &= mask - 1;
    const uint64_t j = j_lo == j_hi ? j_lo : entry_at(S.offset, j_lo, j_hi, p0 + q);
    pos[rank++] = (uint32_t)(p0 + q - S.offset[j]);  // (rank < ops: the build counted these very bytes)
  }
}

struct SliceRows {
  uint64_t n_rows;
  const swg_lift_row* rows;
  uint32_t min_aligned;
  const uint32_t* pos;    // [ops]
  swg_lift_slice* slice;  // [n_rows] written where keep is set
  Plan* plan;             // [n_rows]
  uint8_t* keep;          // [n_rows]
};

__global__ __launch_bounds__(TB) void slice_rows_kernel(SliceRows R, CigarSet S, LiftCols c, unsigned long long* __restrict__ scalars) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  bool interp = false, empty = false, too_short = false, too_long = false;
  if (i < R.n_rows) {
    const uint4* in = reinterpret_cast<const uint4*>(R.rows + i);
    const uint4 a = in[0];  // region, record, ca, cb
    const uint4 b = in[1];  // dst_seq, dst_start, dst_end, flags
    uint64_t lo = 0, hi = S.k;  // the first slot whose record is >= a.y
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (S.record[mid] < a.y) lo = mid + 1;
      else hi = mid;
    }
    bool keep = false;
    if (lo < S.k && S.record[lo] == a.y && reinterpret_cast<const uint8_t*>(S.state)[lo] == 0) {
      const uint32_t first = S.op_first[lo], nops = S.op_first[lo + 1] - first, rec = a.y;
      const uint64_t entry = S.offset[lo];
      too_long = (S.offset[lo + 1] - entry) >> 32 != 0;  // (its letter positions do not fit pos[]: the call is refused)
      Slice s;
      Plan p;
      const uint32_t aligned = too_long ? 0u
                                        : slice_of(S.P, first, nops, R.pos + first, S.text, entry, b.w >> 1 & 1u, b.w & 1u, a.z, a.w, c.start[0][rec],
                                                   c.end[0][rec], c.start[1][rec], &s, &p);
      empty = aligned == 0;
      too_short = aligned != 0 && aligned < R.min_aligned;
      keep = aligned != 0 && !too_short;
      if (keep) {
        uint2* o = reinterpret_cast<uint2*>(R.slice + i);  // 56 bytes: seven 8-byte stores
        o[0] = make_uint2(a.x, a.y);
        o[1] = make_uint2(s.q_start, s.q_end);
        o[2] = make_uint2(s.t_start, s.t_end);
        o[3] = make_uint2((b.w & 3u) | (s.has_eq ? SWG_SLICE_HAS_EQ : 0u), s.aligned);
        o[4] = make_uint2(s.matches, s.text_len);
        o[5] = make_uint2((uint32_t)s.block, (uint32_t)(s.block >> 32));
        o[6] = make_uint2(0u, 0u);
        R.plan[i] = p;
      }
    } else {
      interp = true;
    }
    R.keep[i] = keep ? 1 : 0;
  }
  count_votes(interp, &scalars[L_INTERP]);
  count_votes(empty, &scalars[L_EMPTY]);
  count_votes(too_short, &scalars[L_SHORT]);
  count_votes(too_long, &scalars[L_LONG]);
}

struct SliceOut {
  uint64_t n_slices;
  const uint32_t* list;  // [n_slices] the kept rows, ascending
  swg_lift_slice* slice;  // [n_slices]
  Plan* plan;             // [n_slices]
  uint64_t* text_end;     // [n_slices] the text lengths, then their inclusive sums
};

__global__ __launch_bounds__(TB) void slice_gather_kernel(SliceRows R, SliceOut O) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (s >= O.n_slices) return;
  const uint32_t i = O.list[s];
  const uint2* in = reinterpret_cast<const uint2*>(R.slice + i);
  uint2* o = reinterpret_cast<uint2*>(O.slice + s);
  uint2 w4 = make_uint2(0u, 0u);
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const uint2 w = in[q];
    if (q == 4) w4 = w;
    o[q] = w;
  }
  O.plan[s] = R.plan[i];
  O.text_end[s] = w4.y;  // text_len
}

__global__ __launch_bounds__(TB) void slice_first_kernel(SliceOut O) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (s >= O.n_slices) return;
  O.slice[s].text_first = O.text_end[s] - O.slice[s].text_len;
}

// the first slice in [lo, n) whose text ends behind byte o (there is one)
__device__ __forceinline__ uint64_t slice_at(const uint64_t* __restrict__ text_end, uint64_t n, uint64_t o) {
  uint64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (text_end[mid] > o) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

template <int W>
__global__ __launch_bounds__(TB) void slice_text_kernel(SliceOut O, const char* __restrict__ text, uint64_t text_bytes, char* __restrict__ out) {
  __shared__ uint32_t l_end[MAX_SLOTS];  // where the tile's slices end, relative to the tile (the last one clamped to TILE)
  __shared__ uint64_t l_span[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;
  const uint32_t len = text_bytes - tile0 < (uint64_t)TILE ? (uint32_t)(text_bytes - tile0) : (uint32_t)TILE;
  if (threadIdx.x == 0) l_span[0] = slice_at(O.text_end, O.n_slices, tile0);
  if (threadIdx.x == 64) l_span[1] = slice_at(O.text_end, O.n_slices, tile0 + len - 1);
  __syncthreads();
  const uint64_t sf = l_span[0];
  uint32_t cnt = (uint32_t)(l_span[1] - sf) + 1u;
  if (cnt > (uint32_t)MAX_SLOTS) cnt = MAX_SLOTS;  // (never: every slice has two bytes or more)
  for (uint32_t s = threadIdx.x; s < cnt; s += TB) {
    const uint64_t e = O.text_end[sf + s] - tile0;
    l_end[s] = e < (uint64_t)TILE ? (uint32_t)e : (uint32_t)TILE;
  }
  __syncthreads();
  const uint64_t first0 = sf ? O.text_end[sf - 1] : 0;  // where slice sf begins: at or in front of the tile
#pragma unroll 1
  for (uint32_t base = 0; base < len; base += TB * W) {
    const uint32_t off0 = base + threadIdx.x * W;
    if (off0 >= len) break;
    uint32_t lo = 0, hi = cnt - 1;  // the first slot that ends behind off0
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (l_end[mid] > off0) hi = mid;
      else lo = mid + 1;
    }
    uint32_t slot = lo, packed = 0;
    Plan p = O.plan[sf + slot];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t off = off0 + w;
      if (off >= len) break;
      if (off >= l_end[slot]) {  // the next slice
        while (slot + 1 < cnt && off >= l_end[slot]) ++slot;
        p = O.plan[sf + slot];
      }
      const uint32_t rel = slot ? off - l_end[slot - 1] : (uint32_t)(tile0 + off - first0);
      const uint32_t v = text_byte(p, text, rel);
      if (W == 1) out[tile0 + off] = (char)v;
      else packed |= v << (8 * w);
    }
    if (W == 4) {
      if (off0 + 4 <= len) {
        *reinterpret_cast<uint32_t*>(out + tile0 + off0) = packed;  // (out: an arena block, 16-byte aligned; tile0 and off0: multiples of 4)
      } else {
        for (uint32_t w = 0; off0 + w < len; ++w) out[tile0 + off0 + w] = (char)(packed >> (8 * w));
      }
    }
  }
}

// bytes per lane and store of slice_text: 4 unless the environment asks for the byte form (tools/lift_paf_bench.py measures both)
int text_form() {
  const char* e = std::getenv("SWG_SLICE_TEXT_FORM");
  return e && e[0] == '1' && !e[1] ? 1 : 4;
}

int slice_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
              const swg_cigar_set* cigars, swg_lift_slice_request* req) {
  static const char* const who = "lift_slice";
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL records or request", who);
  if (req->reserved) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: reserved must be 0", who);
  SWG_TRY(swg_lift_check_request(ctx, rec, status, regions, m, req->set, req->axes));
  const uint64_t n = rec->n, k = cigars ? cigars->k : 0;
  const uint32_t n_seq = rec->n_seq;
  uint64_t B = 0;
  SWG_TRY(cigar_set_check_host(ctx, who, cigars, on_device, n, &B));
  req->n_rows = req->n_slices = req->n_interp = req->n_empty = req->n_short = req->text_bytes = req->ops = req->cigar_bad = 0;
  const bool lift = m != 0 && n != 0;
  if (!lift && !k) return SWG_OK;  // no device work
  SWG_TRY(swg_lift_check_columns(ctx, rec, on_device, regions, m));
  const int n_axes = __builtin_popcount(req->axes);
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * (24 * n_axes + (on_device ? 0 : 26)) + (size_t)m * (12 * n_axes + 48) + (size_t)B * 4 + (size_t)k * 24 + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    hipStream_t st = ctx->stream;
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const swg_lift_region* d_regions = regions;
    CigarSet S{};
    S.k = k, S.B = B;
    if (k) S.record = cigars->record, S.offset = cigars->offset, S.text = cigars->text;
    if (!on_device) {
      swg_stager s(ctx);
      swg_lift_stage(&s, n, m, &c, &d_regions);
      if (k) {
        s.add(&S.record, k);
        s.add(&S.offset, k + 1);
        s.add(&S.text, B);
      }
      SWG_TRY(s.run());
    }
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, L_TOTAL);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(scalars, 0, L_TOTAL * sizeof(unsigned long long), st));
    uint64_t* const d_scalars = reinterpret_cast<uint64_t*>(scalars);
    if (k && on_device) SWG_TRY(cigar_set_check_device(ctx, who, n, &S, scalars));
    if (k) SWG_TRY(cigar_build(ctx, who, c, &S, scalars));
    swg_lift_request plain{};
    plain.set = req->set, plain.axes = req->axes;
    LiftDeviceRows dev{};
    dev.always = true;
    if (lift) SWG_TRY(swg_lift_rows_device(ctx, n, n_seq, c, d_regions, m, &plain, &dev));
    const uint64_t n_rows = plain.n;
    if (n_rows >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 rows or more in one call", who);
    uint64_t n_slices = 0, text_bytes = 0;
    if (dev.rows && n_rows && k) {
      SliceRows R{};
      R.n_rows = n_rows, R.rows = dev.rows, R.min_aligned = req->min_aligned;
      uint32_t* pos = swg_alloc<uint32_t>(ctx, S.ops + 1);
      R.slice = swg_alloc<swg_lift_slice>(ctx, n_rows);
      R.plan = swg_alloc<Plan>(ctx, n_rows);
      R.keep = swg_alloc<uint8_t>(ctx, n_rows);
      SWG_CHECK_ARENA(ctx);
      if (S.B) {
        const int aligned = (reinterpret_cast<uintptr_t>(S.text) & 15) == 0;
        SWG_LAUNCH(ctx, "slice_op_pos", slice_op_pos_kernel<<<grid_of((S.B + 15) / 16), TB, 0, st>>>(S, aligned, pos));
        SWG_KERNEL_CHECK(ctx);
      }
      R.pos = pos;
      SWG_LAUNCH(ctx, "slice_rows", slice_rows_kernel<<<grid_of(n_rows), TB, 0, st>>>(R, S, c, scalars));
      SWG_KERNEL_CHECK(ctx);
      swg_flag_scan fs;
      SWG_TRY(swg_flags_count(ctx, R.keep, n_rows, &fs, d_scalars + L_SLICES));
      uint64_t h2[2];  // L_SLICES, L_LONG
      SWG_TRY(swg_read_scalars(ctx, d_scalars + L_SLICES, h2, 2));
      if (h2[1]) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: an entry of 2^32 bytes or more", who);
      n_slices = h2[0];
      if (n_slices) {
        SliceOut O{};
        O.n_slices = n_slices;
        uint32_t* list = swg_alloc<uint32_t>(ctx, n_slices);
        O.slice = swg_alloc<swg_lift_slice>(ctx, n_slices);
        O.plan = swg_alloc<Plan>(ctx, n_slices);
        O.text_end = swg_alloc<uint64_t>(ctx, n_slices);
        SWG_CHECK_ARENA(ctx);
        SWG_TRY(swg_flags_compact(ctx, fs, list));
        O.list = list;
        SWG_LAUNCH(ctx, "slice_gather", slice_gather_kernel<<<grid_of(n_slices), TB, 0, st>>>(R, O));
        SWG_KERNEL_CHECK(ctx);
        SWG_TRY(swg_inclusive_sum_scan_u64(ctx, O.text_end, O.text_end, n_slices));
        SWG_TRY(swg_read_scalars(ctx, O.text_end + (n_slices - 1), &text_bytes, 1));
        if (text_bytes >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of slice text or more in one call", who);
        SWG_LAUNCH(ctx, "slice_first", slice_first_kernel<<<grid_of(n_slices), TB, 0, st>>>(O));
        SWG_KERNEL_CHECK(ctx);
        if (req->text && text_bytes <= req->text_capacity) {
          char* out = swg_alloc<char>(ctx, text_bytes);
          SWG_CHECK_ARENA(ctx);
          const unsigned tiles = (unsigned)((text_bytes + TILE - 1) / TILE);
          if (text_form() == 1) SWG_LAUNCH(ctx, "slice_text", slice_text_kernel<1><<<tiles, TB, 0, st>>>(O, S.text, text_bytes, out));
          else SWG_LAUNCH(ctx, "slice_text", slice_text_kernel<4><<<tiles, TB, 0, st>>>(O, S.text, text_bytes, out));
          SWG_KERNEL_CHECK(ctx);
          SWG_HIP(ctx, hipMemcpyAsync(req->text, out, text_bytes, hipMemcpyDeviceToHost, st));
        }
        if (req->slices && n_slices <= req->slice_capacity)
          SWG_HIP(ctx, hipMemcpyAsync(req->slices, O.slice, n_slices * sizeof(swg_lift_slice), hipMemcpyDeviceToHost, st));
      }
    }
    if (k && req->state) SWG_HIP(ctx, hipMemcpyAsync(req->state, S.state, k, hipMemcpyDeviceToHost, st));
    uint64_t h[L_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, d_scalars, h, L_TOTAL));
    req->n_rows = n_rows, req->n_slices = n_slices, req->text_bytes = text_bytes;
    req->n_interp = k ? h[L_INTERP] : n_rows, req->n_empty = h[L_EMPTY], req->n_short = h[L_SHORT];
    req->ops = S.ops, req->cigar_bad = h[C_BAD_ENTRIES];
    return SWG_OK;
  });
}

}  // namespace

int swg_lift_slice_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                       const swg_cigar_set* cigars, swg_lift_slice_request* req) {
  try {
    return slice_run(ctx, rec, on_device, status, regions, m, cigars, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_lift_slice_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                      const swg_cigar_set* cigars, swg_lift_slice_request* req) {
  return swg_lift_slice_run(ctx, rec, false, status, regions, m, cigars, req);
}
extern "C" int swg_lift_slice_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                             const swg_cigar_set* cigars, swg_lift_slice_request* req) {
  return swg_lift_slice_run(ctx, rec, true, status, regions, m, cigars, req);
}
extern "C" uint32_t swg_lift_slice_text_tile(void) { return SWG_SLICE_TEXT_TILE; }
