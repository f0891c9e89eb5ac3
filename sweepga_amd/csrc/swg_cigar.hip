// Base-exact lift: the CIGARs of the hit records parsed on the device, prefix sums over their ops, and every
// row of the lift refined through them.  The lift itself (hits, clips, order, summary) is swg_lift.hip's, which leaves its rows in the
// arena frame for the kernels here.
//
//   cigar_set_check  (device seam only) one thread per entry: record[] strictly ascending and < n, offset[] from 0 and non-decreasing;
//                    the text length offset[k] is read back with the error word.
//   cigar_count      a tile of 4,096 text bytes per work-group, 16 per thread in one load: a byte that is no digit ends an op (a
//                    letter, or a foreign byte that the parse turns into a syntax error).  The tile's ops are counted.
//   (scan)           swg_inclusive_sum_scan_u64 over the tile counts: tile offsets and the number of ops, which is read back (it sizes
//                    the prefix arrays; 2^31 or more is refused).
//   cigar_parse      the same tile again: the ops are ranked by a wavefront scan plus the work-group's wave counts (flag_compact's
//                    scheme).  Each thread stores the rank of its 16 bytes (entries find their first op there) and each op reads its
//                    own digits back, at most 11 bytes, down to the previous non-digit or to the entry's first byte: a number that
//                    straddles a tile border needs no carry between work-groups.  The op's four advances go to the four arrays at its
//                    rank.  Errors are combined per entry in LDS (slot = the entry's first byte in the tile, 0 for the entry that
//                    reaches in from the left) and leave as one atomic per (work-group, entry).
//   (scan)           swg_inclusive_sum_scan_u64 over each of the four arrays, shifted by one element: exclusive prefix sums over all
//                    ops of the call.  A record's sums are differences against the value at its first op.
//   cigar_entries    one thread per entry: its op range from the chunk ranks, trailing digits, the two totals against the record's
//                    Lq and Lt in 64 bits, the empty state; bad entries are counted with one atomic per wavefront.
//   cigar_refine     one thread per row of the lift: a binary search for the record in record[], and on state 0 four more in the
//                    record's prefix arrays (swg_cigar_walk.h); the 40-byte row is written.  Exact rows are counted per wavefront.
//   hit_mark         (swg_lift_hit_records) flags[record] = 1 for every row, plain stores; swg_flags_count / swg_flags_compact give
//                    the ascending list.
//
// No work-group waits for another inside a launch; every carry goes through the library's scans between launches.
#include <algorithm>
#include <cstring>
#include <new>

#include "swg_internal.h"
#include "swg_lift_index.h"
#include "swg_pair_table.h"
#include "swg_cigar_walk.h"
#include "swg_cigar_build.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;
using namespace swg_lift_ix;
using namespace swg_cigar;

constexpr int CT = TB * 16;  // text bytes per tile
static_assert(TB == 256 && WAVES == 4, "16 bytes per thread, four wavefronts");
// device scalars of a call, behind those of the build
enum { C_EXACT = C_BUILD_TOTAL, C_HITS, C_TOTAL };

// the thread's 16 bytes from position i on; bytes at or behind B read as '0' (a digit: never an op)
__device__ __forceinline__ void load_text16(const char* __restrict__ text, uint64_t i, uint64_t B, bool aligned, uint32_t w[4]) {
  if (aligned && i + 16 <= B) {
    const uint4 q = *reinterpret_cast<const uint4*>(text + i);
    w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint64_t j = i + (uint64_t)k * 4 + b;
        v |= (uint32_t)(j < B ? (unsigned char)text[j] : (unsigned char)'0') << (8 * b);
      }
      w[k] = v;
    }
  }
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t w[4], int b) { return (w[b >> 2] >> (8 * (b & 3))) & 0xffu; }
// bit b: byte b is no digit
__device__ __forceinline__ uint32_t op_mask(const uint32_t w[4]) {
  uint32_t m = 0;
#pragma unroll
  for (int b = 0; b < 16; ++b) m |= (is_digit((unsigned char)byte_of(w, b)) ? 0u : 1u) << b;
  return m;
}

__global__ __launch_bounds__(TB) void cigar_set_check_kernel(uint64_t k, uint64_t n, const uint32_t* __restrict__ record, const uint64_t* __restrict__ offset,
                                                            unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= k) return;
  unsigned long long bad = 0;
  if (record[j] >= n) bad |= 1ull;
  if (j && record[j - 1] >= record[j]) bad |= 2ull;
  if (offset[j + 1] < offset[j] || (j == 0 && offset[0] != 0)) bad |= 4ull;
  if (bad) atomicOr(&scalars[C_BAD], bad);
  if (j == k - 1) scalars[C_BYTES] = offset[k];
}

__global__ __launch_bounds__(TB) void cigar_count_kernel(const char* __restrict__ text, uint64_t B, int aligned, uint64_t* __restrict__ tile_cnt) {
  __shared__ uint32_t l_wave[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t w[4];
  load_text16(text, (uint64_t)blockIdx.x * CT + (uint64_t)threadIdx.x * 16, B, aligned != 0, w);
  uint32_t c = __popc(op_mask(w));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
  if (lane == 0) l_wave[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (uint64_t)l_wave[0] + l_wave[1] + l_wave[2] + l_wave[3];
}

// the last entry j in [lo, hi] with offset[j] <= pos (offset[lo] <= pos)
__device__ __forceinline__ uint64_t entry_of(const uint64_t* __restrict__ offset, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo + 1) >> 1);
    if (offset[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct CigarParse {
  const char* text;
  uint64_t B, k;
  const uint64_t* offset;    // [k + 1]
  const uint64_t* tile_inc;  // [tiles] inclusive scan of the tiles' ops
  uint32_t* chunk_rank;      // [ceil(B / 16)] the ops in front of each 16-byte chunk
  uint64_t *X, *Y, *A, *E;   // [ops] the ops' advances, at their ranks
  uint32_t* state;           // [ceil(k / 4)] the state bytes, four to a word
  int aligned;
};

__global__ __launch_bounds__(TB) void cigar_parse_kernel(CigarParse P) {
  __shared__ uint32_t l_wave[WAVES];
  __shared__ uint32_t l_err[CT];  // per byte of the tile where an entry begins: its error bits ...
  __shared__ uint32_t l_ent[CT];  // ... and the entry
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * CT, p0 = tile0 + (uint64_t)threadIdx.x * 16;
  uint32_t w[4];
  load_text16(P.text, p0, P.B, P.aligned != 0, w);
  const uint32_t mask = op_mask(w), c = __popc(mask);
  uint32_t inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) l_wave[wave] = inc;
#pragma unroll
  for (int s = 0; s < 16; ++s) l_err[threadIdx.x * 16 + s] = 0;
  __syncthreads();
  uint64_t rank = (blockIdx.x ? P.tile_inc[blockIdx.x - 1] : 0) + (inc - c);
  for (int v = 0; v < wave; ++v) rank += l_wave[v];
  if (p0 < P.B) {
    P.chunk_rank[p0 >> 4] = (uint32_t)rank;  // (fewer than 2^31 ops: the host has looked)
    if (mask) {
      const uint64_t last = p0 + 15 < P.B ? p0 + 15 : P.B - 1;
      const uint64_t j_lo = entry_of(P.offset, 0, P.k - 1, p0), j_hi = entry_of(P.offset, j_lo, P.k - 1, last);
      uint32_t m = mask;
      while (m) {
        const int b = __builtin_ctz(m);
        m &= m - 1;
        const uint64_t pos = p0 + b;
        const uint64_t j = j_lo == j_hi ? j_lo : entry_of(P.offset, j_lo, j_hi, pos);
        const uint64_t first = P.offset[j];
        uint32_t len;
        uint32_t err = op_number(P.text, first, pos, &len);
        uint64_t dx, dy, da, de;
        const uint32_t foreign = op_advance((unsigned char)byte_of(w, b), len, &dx, &dy, &da, &de);
        if (foreign) err = foreign;
        P.X[rank] = dx, P.Y[rank] = dy, P.A[rank] = da, P.E[rank] = de;
        ++rank;
        if (err) {
          const uint32_t slot = first > tile0 ? (uint32_t)(first - tile0) : 0u;
          l_ent[slot] = (uint32_t)j;  // (every writer of a slot writes the same entry)
          atomicOr(&l_err[slot], err);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < 16; ++s) {  // one atomic per (work-group, entry with an error)
    const uint32_t err = l_err[threadIdx.x * 16 + s];
    if (!err) continue;
    const uint32_t j = l_ent[threadIdx.x * 16 + s];
    atomicOr(&P.state[j >> 2], err << (8 * (j & 3u)));
  }
}

__global__ __launch_bounds__(TB) void cigar_entries_kernel(CigarSet S, LiftCols c, unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  bool bad = false;
  if (j < S.k) {
    const uint64_t o0 = S.offset[j], o1 = S.offset[j + 1];
    const uint32_t f = rank_at(S, o0), l = rank_at(S, o1);
    S.op_first[j] = f;
    if (j == S.k - 1) S.op_first[S.k] = l;
    const uint32_t shift = 8 * (uint32_t)(j & 3);
    uint32_t st = 0;
    if (o0 == o1) {
      st = ST_EMPTY;
    } else {
      const uint32_t parsed = (S.state[j >> 2] >> shift) & 0xffu;  // (this byte: written by cigar_parse, before this launch)
      if (is_digit((unsigned char)S.text[o1 - 1])) st |= ST_SYNTAX;
      if (!((st | parsed) & (ST_SYNTAX | ST_VALUE))) {
        const uint32_t rec = S.record[j];
        if (S.P.X[l] - S.P.X[f] != (uint64_t)(c.end[0][rec] - c.start[0][rec])) st |= ST_QSUM;
        if (S.P.Y[l] - S.P.Y[f] != (uint64_t)(c.end[1][rec] - c.start[1][rec])) st |= ST_TSUM;
      }
      bad = ((st | parsed) & 15u) != 0;
    }
    if (st) atomicOr(&S.state[j >> 2], st << shift);
  }
  const uint64_t votes = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&scalars[C_BAD_ENTRIES], (unsigned long long)__popcll(votes));
}

__global__ __launch_bounds__(TB) void cigar_refine_kernel(uint64_t n_rows, const swg_lift_row* __restrict__ rows, swg_lift_exact_row* __restrict__ out,
                                                         CigarSet S, LiftCols c, unsigned long long* __restrict__ scalars) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  bool exact = false;
  if (i < n_rows) {
    const uint4* in = reinterpret_cast<const uint4*>(rows + i);
    const uint4 a = in[0];  // region, record, ca, cb
    uint4 b = in[1];        // dst_seq, dst_start, dst_end, flags
    uint32_t aligned = 0, matches = 0;
    uint64_t lo = 0, hi = S.k;  // the first slot whose record is >= a.y
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (S.record[mid] < a.y) lo = mid + 1;
      else hi = mid;
    }
    if (lo < S.k && S.record[lo] == a.y && reinterpret_cast<const uint8_t*>(S.state)[lo] == 0) {
      const uint32_t first = S.op_first[lo], nops = S.op_first[lo + 1] - first, rec = a.y;
      refine(S.P, first, nops, b.w >> 1 & 1u, b.w & 1u, a.z, a.w, c.start[0][rec], c.end[0][rec], c.start[1][rec], c.end[1][rec], &b.y, &b.z, &aligned,
             &matches);
      b.w |= SWG_LIFT_EXACT;
      exact = true;
    }
    uint2* o = reinterpret_cast<uint2*>(out + i);  // 40 bytes: five 8-byte stores
    o[0] = make_uint2(a.x, a.y);
    o[1] = make_uint2(a.z, a.w);
    o[2] = make_uint2(b.x, b.y);
    o[3] = make_uint2(b.z, b.w);
    o[4] = make_uint2(aligned, matches);
  }
  const uint64_t votes = __ballot(exact);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&scalars[C_EXACT], (unsigned long long)__popcll(votes));
}

__global__ __launch_bounds__(TB) void hit_mark_kernel(uint64_t n_rows, const swg_lift_row* __restrict__ rows, uint8_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i < n_rows) flags[rows[i].record] = 1;
}

int bad_set(swg_ctx* ctx, const char* who, uint64_t bad) {
  if (bad & 1u) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: a record of the CIGAR set is >= n", who);
  if (bad & 2u) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the records of the CIGAR set are not strictly ascending", who);
  if (bad & 4u) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the offsets of the CIGAR set do not start at 0 or decrease", who);
  return SWG_OK;
}

unsigned grid_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

}  // namespace

namespace swg_cigar {

int cigar_set_check_host(swg_ctx* ctx, const char* who, const swg_cigar_set* cigars, bool on_device, uint64_t n, uint64_t* B) {
  const uint64_t k = cigars ? cigars->k : 0;
  *B = 0;
  if (k >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^31 entries or more in one call", who);
  if (k && (!cigars->record || !cigars->offset)) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL record or offset array of the CIGAR set", who);
  if (k && n == 0) return bad_set(ctx, who, 1);  // (any record is >= n)
  if (k && !on_device) {  // the set is here: its faults cost no device work
    uint64_t bad = cigars->offset[0] != 0 ? 4u : 0u;
    for (uint64_t j = 0; j < k; ++j)
      bad |= (cigars->record[j] >= n ? 1u : 0u) | (j && cigars->record[j - 1] >= cigars->record[j] ? 2u : 0u) |
             (cigars->offset[j + 1] < cigars->offset[j] ? 4u : 0u);
    SWG_TRY(bad_set(ctx, who, bad));
    *B = cigars->offset[k];
    if (*B && !cigars->text) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL text of the CIGAR set", who);
  }
  return SWG_OK;
}

int cigar_set_check_device(swg_ctx* ctx, const char* who, uint64_t n, CigarSet* S, unsigned long long* scalars) {
  uint64_t h[2];
  SWG_LAUNCH(ctx, "cigar_set_check", cigar_set_check_kernel<<<grid_of(S->k), TB, 0, ctx->stream>>>(S->k, n, S->record, S->offset, scalars));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 2));
  SWG_TRY(bad_set(ctx, who, h[C_BAD]));
  S->B = h[C_BYTES];
  if (S->B && !S->text) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL text of the CIGAR set", who);
  return SWG_OK;
}

// Parse, prefix sums and entry states of a set whose arrays are in device memory (inside an arena frame).  B: the text's length.
int cigar_build(swg_ctx* ctx, const char* who, const LiftCols& c, CigarSet* S, unsigned long long* scalars) {
  hipStream_t st = ctx->stream;
  const uint64_t k = S->k, B = S->B;
  const uint64_t state_words = (k + 3) / 4;
  S->state = swg_alloc<uint32_t>(ctx, state_words);
  S->op_first = swg_alloc<uint32_t>(ctx, k + 1);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(S->state, 0, state_words * sizeof(uint32_t), st));
  S->ops = 0;
  uint64_t* prefix[4] = {nullptr, nullptr, nullptr, nullptr};
  if (B) {
    const uint64_t tiles = (B + CT - 1) / CT;
    if (tiles >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^43 bytes of CIGAR text or more in one call", who);
    uint64_t* tile_inc = swg_alloc<uint64_t>(ctx, tiles);
    uint32_t* chunk_rank = swg_alloc<uint32_t>(ctx, (B + 15) / 16);
    SWG_CHECK_ARENA(ctx);
    const int aligned = (reinterpret_cast<uintptr_t>(S->text) & 15) == 0;
    SWG_LAUNCH(ctx, "cigar_count", cigar_count_kernel<<<(unsigned)tiles, TB, 0, st>>>(S->text, B, aligned, tile_inc));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_inclusive_sum_scan_u64(ctx, tile_inc, tile_inc, tiles));
    SWG_TRY(swg_read_scalars(ctx, tile_inc + (tiles - 1), &S->ops, 1));  // sizes the prefix arrays
    if (S->ops >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^31 ops or more in one call", who);
    // ops + 1 sums per array, the values from element 1 on: element 1 sits on a 16-byte boundary for the scan's wide loads
    for (auto& p : prefix) p = swg_alloc<uint64_t>(ctx, S->ops + 2) + 1;
    SWG_CHECK_ARENA(ctx);
    for (auto& p : prefix) SWG_HIP(ctx, hipMemsetAsync(p, 0, sizeof(uint64_t), st));
    CigarParse P{S->text, B, k, S->offset, tile_inc, chunk_rank, prefix[0] + 1, prefix[1] + 1, prefix[2] + 1, prefix[3] + 1, S->state, aligned};
    SWG_LAUNCH(ctx, "cigar_parse", cigar_parse_kernel<<<(unsigned)tiles, TB, 0, st>>>(P));
    SWG_KERNEL_CHECK(ctx);
    for (auto& p : prefix) SWG_TRY(swg_inclusive_sum_scan_u64(ctx, p + 1, p + 1, S->ops));
    S->chunk_rank = chunk_rank;
  } else {  // every entry is empty: nothing is read through these
    for (auto& p : prefix) p = swg_alloc<uint64_t>(ctx, 1);
    SWG_CHECK_ARENA(ctx);
    S->chunk_rank = nullptr;
  }
  S->P = Prefix{prefix[0], prefix[1], prefix[2], prefix[3]};
  SWG_LAUNCH(ctx, "cigar_entries", cigar_entries_kernel<<<grid_of(k), TB, 0, st>>>(*S, c, scalars));
  SWG_KERNEL_CHECK(ctx);
  return SWG_OK;
}

}  // namespace swg_cigar

namespace {

int exact_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
              const swg_cigar_set* cigars, swg_lift_exact_request* req) {
  static_assert(sizeof(swg_cigar_set) == 32 && sizeof(swg_lift_exact_row) == 40 && sizeof(swg_lift_exact_request) == 88, "the ABI's sizes");
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "lift_exact: NULL records or request");
  SWG_TRY(swg_lift_check_request(ctx, rec, status, regions, m, req->set, req->axes));
  const uint64_t n = rec->n, k = cigars ? cigars->k : 0;
  const uint32_t n_seq = rec->n_seq;
  uint64_t B = 0;
  SWG_TRY(cigar_set_check_host(ctx, "lift_exact", cigars, on_device, n, &B));
  req->n = 0;
  req->candidates[0] = req->candidates[1] = 0;
  req->ops = req->cigar_bad = req->exact_rows = 0;
  const bool lift = m != 0 && n != 0;
  if (!lift && req->summary && m) std::memset(req->summary, 0, m * sizeof(swg_lift_summary));
  if (!lift && !k) return SWG_OK;  // no device work
  SWG_TRY(swg_lift_check_columns(ctx, rec, on_device, regions, m));
  const int n_axes = __builtin_popcount(req->axes);
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * (24 * n_axes + (on_device ? 0 : 26)) + (size_t)m * (12 * n_axes + 48) + (size_t)B * 3 + (size_t)k * 24 + (size_t(4) << 20)));
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
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, C_TOTAL);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(scalars, 0, C_TOTAL * sizeof(unsigned long long), st));
    uint64_t h[C_TOTAL];
    if (k && on_device) SWG_TRY(cigar_set_check_device(ctx, "lift_exact", n, &S, scalars));
    if (k) SWG_TRY(cigar_build(ctx, "lift_exact", c, &S, scalars));
    swg_lift_request plain{};
    plain.set = req->set, plain.axes = req->axes;
    plain.capacity = req->capacity;
    plain.rows = req->rows ? reinterpret_cast<swg_lift_row*>(req->rows) : nullptr;  // (only looked at as "rows are wanted")
    plain.summary = req->summary;
    LiftDeviceRows dev{};
    if (lift) SWG_TRY(swg_lift_rows_device(ctx, n, n_seq, c, d_regions, m, &plain, &dev));
    if (dev.rows) {
      swg_lift_exact_row* out = swg_alloc<swg_lift_exact_row>(ctx, plain.n);
      SWG_CHECK_ARENA(ctx);
      SWG_LAUNCH(ctx, "cigar_refine", cigar_refine_kernel<<<grid_of(plain.n), TB, 0, st>>>(plain.n, dev.rows, out, S, c, scalars));
      SWG_KERNEL_CHECK(ctx);
      SWG_HIP(ctx, hipMemcpyAsync(req->rows, out, plain.n * sizeof(swg_lift_exact_row), hipMemcpyDeviceToHost, st));
    }
    if (k && req->state) SWG_HIP(ctx, hipMemcpyAsync(req->state, S.state, k, hipMemcpyDeviceToHost, st));
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, C_TOTAL));
    req->n = plain.n;
    req->candidates[0] = plain.candidates[0], req->candidates[1] = plain.candidates[1];
    req->ops = S.ops, req->cigar_bad = h[C_BAD_ENTRIES], req->exact_rows = h[C_EXACT];
    return SWG_OK;
  });
}

int hit_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m, uint32_t set,
            uint32_t axes, uint32_t* out, uint64_t capacity, uint64_t* k_out) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !k_out) return swg_set_error(ctx, SWG_ERR_INVALID, "lift_hit_records: NULL records or count");
  SWG_TRY(swg_lift_check_request(ctx, rec, status, regions, m, set, axes));
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  *k_out = 0;
  if (m == 0 || n == 0) return SWG_OK;  // no device work
  SWG_TRY(swg_lift_check_columns(ctx, rec, on_device, regions, m));
  const int n_axes = __builtin_popcount(axes);
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * (24 * n_axes + (on_device ? 1 : 27)) + (size_t)m * (12 * n_axes + 48) + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    hipStream_t st = ctx->stream;
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const swg_lift_region* d_regions = regions;
    if (!on_device) {
      swg_stager s(ctx);
      swg_lift_stage(&s, n, m, &c, &d_regions);
      SWG_TRY(s.run());
    }
    swg_lift_request plain{};
    plain.set = set, plain.axes = axes;
    LiftDeviceRows dev{};
    dev.always = true;
    SWG_TRY(swg_lift_rows_device(ctx, n, n_seq, c, d_regions, m, &plain, &dev));
    if (!dev.rows) return SWG_OK;  // no row: no record
    uint8_t* flags = swg_alloc<uint8_t>(ctx, n);
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, C_TOTAL);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(flags, 0, n, st));
    SWG_LAUNCH(ctx, "hit_mark", hit_mark_kernel<<<grid_of(plain.n), TB, 0, st>>>(plain.n, dev.rows, flags));
    SWG_KERNEL_CHECK(ctx);
    swg_flag_scan fs;
    SWG_TRY(swg_flags_count(ctx, flags, n, &fs, reinterpret_cast<uint64_t*>(scalars) + C_HITS));
    uint64_t hits = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + C_HITS, &hits, 1));
    *k_out = hits;
    if (out && hits <= capacity) {
      uint32_t* list = swg_alloc<uint32_t>(ctx, hits);
      SWG_CHECK_ARENA(ctx);
      SWG_TRY(swg_flags_compact(ctx, fs, list));
      SWG_HIP(ctx, hipMemcpyAsync(out, list, hits * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));
    }
    return SWG_OK;
  });
}

}  // namespace

int swg_lift_exact_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                       const swg_cigar_set* cigars, swg_lift_exact_request* req) {
  try {
    return exact_run(ctx, rec, on_device, status, regions, m, cigars, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

int swg_lift_hit_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                     uint32_t set, uint32_t axes, uint32_t* out, uint64_t capacity, uint64_t* k) {
  try {
    return hit_run(ctx, rec, on_device, status, regions, m, set, axes, out, capacity, k);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_lift_exact_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                      const swg_cigar_set* cigars, swg_lift_exact_request* req) {
  return swg_lift_exact_run(ctx, rec, false, status, regions, m, cigars, req);
}
extern "C" int swg_lift_exact_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                             const swg_cigar_set* cigars, swg_lift_exact_request* req) {
  return swg_lift_exact_run(ctx, rec, true, status, regions, m, cigars, req);
}
extern "C" int swg_lift_hit_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                    uint32_t set, uint32_t axes, uint32_t* out, uint64_t capacity, uint64_t* k) {
  return swg_lift_hit_run(ctx, rec, false, status, regions, m, set, axes, out, capacity, k);
}
extern "C" int swg_lift_hit_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_lift_region* regions, uint64_t m,
                                           uint32_t set, uint32_t axes, uint32_t* out, uint64_t capacity, uint64_t* k) {
  return swg_lift_hit_run(ctx, rec, true, status, regions, m, set, axes, out, capacity, k);
}
