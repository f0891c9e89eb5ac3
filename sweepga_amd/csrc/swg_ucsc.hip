// UCSC chain files: one chain per record from its CIGAR -- the ungapped blocks, the differences between their
// starts and the decimal block lines, all on the device.  The parse, the four prefix sums, op_first[] and the entry states are
// cigar_build's (swg_cigar.hip, swg_cigar_build.h); include/sweepga_gpu.h states the definitions, swg_ucsc_walk.h holds the rules.
//
//   ucsc_entries  one thread per entry: the state with bit 32 (a record that ends beyond its sequence), and into the flag byte of
//                 the entry's first op its border: 2, or 3 when the entry gives no chain (state != 0, or its record is outside the
//                 set).  Entries without ops write nothing, so every byte has one writer.
//   ucsc_mark     a tile of 1,024 ops per work-group, 4 consecutive ones per thread: aligned / advancing from the prefix differences,
//                 and the tile maxima of the two marks (swg_ucsc_walk.h): the last advancing op and the last border.
//   (scan)        swg_inclusive_max_scan_u64 over each set of tile maxima: the carry across work-groups, no wait inside a launch.
//   ucsc_starts   the tile again: the running maxima in front of every op (running_max_before, swg_union_tiles.h), the block-start
//                 flag into the op's flag byte.  A run of zero-length ops of any length carries through: they raise no mark.
//   (compaction)  swg_flags_count / swg_flags_compact: the block starts, ascending; their number is read back (it sizes the outputs).
//   ucsc_chains   one thread per entry: its blocks by two searches in the starts, the chain's ends, score and strand; 48-byte row.
//   ucsc_blocks   one thread per OUTPUT block: its entry by a search in op_first[], then size, dt, dq with the swap's index and
//                 field mapping (block_of), 12 bytes, and the length of its line from digit counts.
//   (scan)        swg_inclusive_sum_scan_u64 over the line lengths: the byte offsets, and the text's length (read back).
//   ucsc_offsets  one thread per entry: text_first of its row.
//   ucsc_format   one thread per block: its line, written byte by byte at its offset.
#include <algorithm>
#include <cstring>
#include <new>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_union_tiles.h"
#include "swg_cigar_build.h"
#include "swg_ucsc_walk.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;   // TB, WAVES, reserve_first
using namespace swg_union_tiles;  // ITEMS, TILE, max64, running_max_before
using swg_lift_ix::LiftCols;
using namespace swg_cigar;
using namespace swg_ucsc;

static_assert(TILE == 1024 && ITEMS == 4, "four ops per thread");
static_assert(sizeof(swg_ucsc_block) == 12 && sizeof(swg_ucsc_chain) == 48 && sizeof(swg_ucsc_request) == 120 && sizeof(swg_ucsc_counts) == 64,
              "include/sweepga_gpu.h states these sizes");
enum { U_BEYOND = C_BUILD_TOTAL, U_BLOCKS, U_CHAINS, U_EMPTY, U_TOTAL };

unsigned grid_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

__device__ __forceinline__ void count_votes(bool vote, unsigned long long* slot) {
  const uint64_t votes = __ballot(vote);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(slot, (unsigned long long)__popcll(votes));
}

__global__ __launch_bounds__(TB) void ucsc_entries_kernel(CigarSet S, LiftCols c, const uint32_t* __restrict__ seq_len, uint32_t n_seq, uint32_t set,
                                                          uint8_t* __restrict__ flags, unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  bool beyond = false;
  if (j < S.k) {
    uint8_t* state = reinterpret_cast<uint8_t*>(S.state);
    const uint32_t rec = S.record[j], q = c.id[0][rec], t = c.id[1][rec];
    // (an id that names no sequence has no length to end within)
    beyond = q >= n_seq || t >= n_seq || c.end[0][rec] > seq_len[q] || c.end[1][rec] > seq_len[t];
    uint32_t st = state[j];  // (this byte: final since cigar_entries, a launch ago)
    if (beyond) state[j] = (uint8_t)(st |= ST_BEYOND);
    const uint32_t first = S.op_first[j];
    if (S.op_first[j + 1] != first) {
      const bool in_set = set == SWG_IV_ALL || c.status[rec] != 0;
      flags[first] = st == 0 && in_set ? BORDER : BORDER_DEAD;
    }
  }
  count_votes(beyond, &scalars[U_BEYOND]);
}

// a thread's ITEMS ops from r0 on: bit 0 aligned, bit 1 advancing, and the flag byte; ops at or behind `ops` read as nothing
__device__ __forceinline__ void load_ops(const Prefix& P, const uint8_t* __restrict__ flags, uint64_t ops, uint64_t r0, uint32_t (&kind)[ITEMS],
                                         uint8_t (&f)[ITEMS]) {
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const uint64_t r = r0 + j;
    kind[j] = 0, f[j] = 0;
    if (r >= ops) continue;
    kind[j] = (op_aligned(P, r) ? 1u : 0u) | (op_advances(P, r) ? 2u : 0u);
    f[j] = flags[r];
  }
}

__global__ __launch_bounds__(TB) void ucsc_mark_kernel(Prefix P, const uint8_t* __restrict__ flags, uint64_t ops, uint64_t ntiles,
                                                       unsigned long long* __restrict__ tile_max) {
  __shared__ unsigned long long l_max[2][WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t r0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint32_t kind[ITEMS];
  uint8_t f[ITEMS];
  load_ops(P, flags, ops, r0, kind, f);
  unsigned long long adv = 0, border = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (kind[j] & 2u) adv = mark_of(r0 + j, kind[j] & 1u);  // (the marks grow with the position: the last one is the maximum)
    if (f[j]) border = mark_of(r0 + j, f[j] & 1u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    adv = max64(adv, __shfl_xor(adv, d));
    border = max64(border, __shfl_xor(border, d));
  }
  if (lane == 0) l_max[0][wave] = adv, l_max[1][wave] = border;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long t = 0;
    for (int w = 0; w < WAVES; ++w) t = max64(t, l_max[threadIdx.x][w]);
    tile_max[threadIdx.x * ntiles + blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(TB) void ucsc_starts_kernel(Prefix P, uint8_t* __restrict__ flags, uint64_t ops, uint64_t ntiles,
                                                         const unsigned long long* __restrict__ carry) {
  __shared__ unsigned long long l_wave[2][WAVES];
  const uint64_t r0 = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
  uint32_t kind[ITEMS];
  uint8_t f[ITEMS];
  load_ops(P, flags, ops, r0, kind, f);
  unsigned long long mine[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (kind[j] & 2u) mine[0] = mark_of(r0 + j, kind[j] & 1u);
    if (f[j]) mine[1] = mark_of(r0 + j, f[j] & 1u);
  }
  unsigned long long front[2];
  running_max_before<2>(mine, l_wave, carry, ntiles, 3u, front);
  unsigned long long adv = front[0], border = front[1];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const uint64_t r = r0 + j;
    if (r >= ops) continue;
    if (f[j]) border = mark_of(r, f[j] & 1u);
    // (the first op of the call lies on a border: border is never 0 where it is looked at)
    flags[r] = is_block_start((kind[j] & 1u) != 0, adv, border) ? 1 : 0;
    if (kind[j] & 2u) adv = mark_of(r, kind[j] & 1u);
  }
}

// the first position of a[0 .. n) whose value is >= v (n when none)
__device__ __forceinline__ uint64_t lower_bound32(const uint32_t* __restrict__ a, uint64_t n, uint32_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct UcscOut {
  const uint32_t* starts;  // [n_blocks] the block starts, ascending op positions
  uint64_t n_blocks;
  swg_ucsc_chain* chains;  // [k]
  swg_ucsc_block* blocks;  // [n_blocks]
  uint64_t* line_end;      // [n_blocks] the lines' lengths, then their inclusive sums
  char* text;
};

__global__ __launch_bounds__(TB) void ucsc_chains_kernel(CigarSet S, LiftCols c, const uint32_t* __restrict__ seq_len, uint32_t set, uint32_t from,
                                                         UcscOut O, unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  bool chain = false, empty = false;
  if (j < S.k) {
    const uint32_t rec = S.record[j], st = reinterpret_cast<const uint8_t*>(S.state)[j];
    const bool minus = c.strand[rec] != 0;
    uint32_t w[8] = {rec, (minus ? SWG_UCSC_MINUS : 0u) | st << 8, 0, 0, 0, 0, 0, 0};
    uint64_t fb = 0;
    if (st == 0 && (set == SWG_IV_ALL || c.status[rec] != 0)) {
      const uint32_t first = S.op_first[j], e = S.op_first[j + 1];
      fb = lower_bound32(O.starts, O.n_blocks, first);
      const uint32_t B = (uint32_t)(lower_bound32(O.starts + fb, O.n_blocks - fb, e));  // (first <= e)
      chain = B != 0, empty = B == 0;
      if (B) {
        const Prefix& P = S.P;
        const uint32_t s0 = O.starts[fb], sl = O.starts[fb + B - 1];
        const uint64_t last = P.A[e] - P.A[sl];
        const uint64_t eq = P.E[e] - P.E[first];
        chain_ends(minus, from == SWG_UCSC_FROM_QUERY, c.start[0][rec], c.end[0][rec], c.start[1][rec], seq_len[c.id[0][rec]], seq_len[c.id[1][rec]],
                   P.X[s0] - P.X[first], P.X[sl] - P.X[first] + last, P.Y[s0] - P.Y[first], P.Y[sl] - P.Y[first] + last, &w[2], &w[3], &w[4], &w[5]);
        w[6] = (uint32_t)(eq ? eq : P.A[e] - P.A[first]);
        w[7] = B;
      } else {
        fb = 0;
      }
    }
    uint4* o = reinterpret_cast<uint4*>(O.chains + j);  // 48 bytes: three 16-byte stores (arena blocks are 16-byte aligned)
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o[2] = make_uint4((uint32_t)fb, (uint32_t)(fb >> 32), 0u, 0u);
  }
  count_votes(chain, &scalars[U_CHAINS]);
  count_votes(empty, &scalars[U_EMPTY]);
}

__global__ __launch_bounds__(TB) void ucsc_blocks_kernel(CigarSet S, uint32_t from, UcscOut O) {
  const uint64_t b = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (b >= O.n_blocks) return;
  // the last entry whose first op is at or in front of the start that sits at this output position: the chain's blocks are
  // blocks [first_block, first_block + n_blocks) in either order, so the start at position b lies in the chain that block b is in
  uint64_t lo = 0, hi = S.k - 1;
  const uint32_t s = O.starts[b];
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo + 1) >> 1);
    if (S.op_first[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  const swg_ucsc_chain& ch = O.chains[lo];
  const uint32_t B = ch.n_blocks, p = (uint32_t)(b - ch.first_block);
  const bool swapped = from == SWG_UCSC_FROM_QUERY, reversed = swapped && (ch.flags & SWG_UCSC_MINUS);
  uint32_t size, dt, dq;
  block_of(S.P, O.starts + ch.first_block, B, S.op_first[lo + 1], p, reversed, swapped, &size, &dt, &dq);
  uint32_t* o = reinterpret_cast<uint32_t*>(O.blocks + b);
  o[0] = size, o[1] = dt, o[2] = dq;
  O.line_end[b] = line_length(size, dt, dq, p + 1 == B);
}

__global__ __launch_bounds__(TB) void ucsc_offsets_kernel(uint64_t k, UcscOut O) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (j >= k) return;
  const swg_ucsc_chain& ch = O.chains[j];
  if (ch.n_blocks && ch.first_block) O.chains[j].text_first = O.line_end[ch.first_block - 1];
}

__global__ __launch_bounds__(TB) void ucsc_format_kernel(UcscOut O) {
  const uint64_t b = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (b >= O.n_blocks) return;
  const uint64_t at = b ? O.line_end[b - 1] : 0;
  const swg_ucsc_block v = O.blocks[b];
  const uint32_t len = (uint32_t)(O.line_end[b] - at);
  // (a chain's last block is the one whose line is `size\n\n`: shorter than any line with three numbers of its size)
  line_text(O.text + at, v.size, v.dt, v.dq, len == digits10(v.size) + 2u);
}

int ucsc_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint8_t* status, const swg_cigar_set* cigars,
             swg_ucsc_request* req) {
  static const char* const who = "ucsc_chain";
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL records or request", who);
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (req->from > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: from must be SWG_UCSC_FROM_TARGET or SWG_UCSC_FROM_QUERY", who);
  if (req->set == SWG_IV_KEPT && !status) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (!seq_len) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL seq_len (the '-' strand needs the sizes)", who);
  const uint64_t n = rec->n, k = cigars ? cigars->k : 0;
  const uint32_t n_seq = rec->n_seq;
  uint64_t B = 0;
  SWG_TRY(cigar_set_check_host(ctx, who, cigars, on_device, n, &B));
  if (B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
  if (k && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL column", who);
  req->n_chains = req->n_blocks = req->text_bytes = req->ops = req->cigar_bad = req->beyond = req->empty_chains = 0;
  if (!k) return SWG_OK;  // no device work
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)(on_device ? 0 : n * 26 + (size_t)n_seq * 4) + (size_t)B * 24 + (size_t)k * 72 + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    hipStream_t st = ctx->stream;
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const uint32_t* d_len = seq_len;  // (the frame may run twice: what the stager replaces is the frame's own)
    CigarSet S{};
    S.k = k, S.B = B;
    S.record = cigars->record, S.offset = cigars->offset, S.text = cigars->text;
    if (!on_device) {
      swg_stager s(ctx);
      for (int a = 0; a < 2; ++a) s.add(&c.id[a], n), s.add(&c.start[a], n), s.add(&c.end[a], n);
      s.add(&c.strand, n);
      s.add(&c.status, n);
      s.add(&d_len, (size_t)n_seq);
      s.add(&S.record, k);
      s.add(&S.offset, k + 1);
      s.add(&S.text, B);
      SWG_TRY(s.run());
    }
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, U_TOTAL);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(scalars, 0, U_TOTAL * sizeof(unsigned long long), st));
    if (on_device) {
      SWG_TRY(cigar_set_check_device(ctx, who, n, &S, scalars));
      if (S.B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
    }
    SWG_TRY(cigar_build(ctx, who, c, &S, scalars));
    const uint64_t ops = S.ops, ntiles = (ops + TILE - 1) / TILE;
    UcscOut O{};
    O.chains = swg_alloc<swg_ucsc_chain>(ctx, k);
    uint8_t* flags = swg_alloc<uint8_t>(ctx, ops + 1);
    unsigned long long* tile_max = swg_alloc<unsigned long long>(ctx, 2 * ntiles + 1);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(flags, 0, ops + 1, st));
    SWG_LAUNCH(ctx, "ucsc_entries", ucsc_entries_kernel<<<grid_of(k), TB, 0, st>>>(S, c, d_len, n_seq, req->set, flags, scalars));
    SWG_KERNEL_CHECK(ctx);
    uint64_t n_blocks = 0;
    if (ops) {
      SWG_LAUNCH(ctx, "ucsc_mark", ucsc_mark_kernel<<<(unsigned)ntiles, TB, 0, st>>>(S.P, flags, ops, ntiles, tile_max));
      SWG_KERNEL_CHECK(ctx);
      for (int s = 0; s < 2; ++s)
        SWG_TRY(swg_inclusive_max_scan_u64(ctx, reinterpret_cast<uint64_t*>(tile_max) + s * ntiles, reinterpret_cast<uint64_t*>(tile_max) + s * ntiles, ntiles));
      SWG_LAUNCH(ctx, "ucsc_starts", ucsc_starts_kernel<<<(unsigned)ntiles, TB, 0, st>>>(S.P, flags, ops, ntiles, tile_max));
      SWG_KERNEL_CHECK(ctx);
      swg_flag_scan fs;
      SWG_TRY(swg_flags_count(ctx, flags, ops, &fs, reinterpret_cast<uint64_t*>(scalars) + U_BLOCKS));
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + U_BLOCKS, &n_blocks, 1));  // sizes the outputs
      if (n_blocks >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^31 blocks or more in one call", who);
      uint32_t* starts = swg_alloc<uint32_t>(ctx, n_blocks + 1);
      SWG_CHECK_ARENA(ctx);
      if (n_blocks) SWG_TRY(swg_flags_compact(ctx, fs, starts));
      O.starts = starts;
    }
    O.n_blocks = n_blocks;
    SWG_LAUNCH(ctx, "ucsc_chains", ucsc_chains_kernel<<<grid_of(k), TB, 0, st>>>(S, c, d_len, req->set, req->from, O, scalars));
    SWG_KERNEL_CHECK(ctx);
    uint64_t text_bytes = 0;
    if (n_blocks) {
      O.blocks = swg_alloc<swg_ucsc_block>(ctx, n_blocks);
      O.line_end = swg_alloc<uint64_t>(ctx, n_blocks);
      SWG_CHECK_ARENA(ctx);
      SWG_LAUNCH(ctx, "ucsc_blocks", ucsc_blocks_kernel<<<grid_of(n_blocks), TB, 0, st>>>(S, req->from, O));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, O.line_end, O.line_end, n_blocks));
      SWG_TRY(swg_read_scalars(ctx, O.line_end + (n_blocks - 1), &text_bytes, 1));
      SWG_LAUNCH(ctx, "ucsc_offsets", ucsc_offsets_kernel<<<grid_of(k), TB, 0, st>>>(k, O));
      SWG_KERNEL_CHECK(ctx);
      if (req->text && text_bytes <= req->text_capacity) {
        O.text = swg_alloc<char>(ctx, text_bytes);
        SWG_CHECK_ARENA(ctx);
        SWG_LAUNCH(ctx, "ucsc_format", ucsc_format_kernel<<<grid_of(n_blocks), TB, 0, st>>>(O));
        SWG_KERNEL_CHECK(ctx);
        SWG_HIP(ctx, hipMemcpyAsync(req->text, O.text, text_bytes, hipMemcpyDeviceToHost, st));
      }
      if (req->blocks && n_blocks <= req->block_capacity)
        SWG_HIP(ctx, hipMemcpyAsync(req->blocks, O.blocks, n_blocks * sizeof(swg_ucsc_block), hipMemcpyDeviceToHost, st));
    }
    if (req->chains && k <= req->chain_capacity) SWG_HIP(ctx, hipMemcpyAsync(req->chains, O.chains, k * sizeof(swg_ucsc_chain), hipMemcpyDeviceToHost, st));
    if (req->state) SWG_HIP(ctx, hipMemcpyAsync(req->state, S.state, k, hipMemcpyDeviceToHost, st));
    uint64_t h[U_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, U_TOTAL));
    req->n_chains = h[U_CHAINS], req->n_blocks = n_blocks, req->text_bytes = text_bytes, req->ops = ops;
    req->cigar_bad = h[C_BAD_ENTRIES], req->beyond = h[U_BEYOND], req->empty_chains = h[U_EMPTY];
    return SWG_OK;
  });
}

}  // namespace

int swg_ucsc_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint8_t* status, const swg_cigar_set* cigars,
                 swg_ucsc_request* req) {
  try {
    return ucsc_run(ctx, rec, on_device, seq_len, status, cigars, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

// What a batch of the PAF seam may hold of CIGAR text by default: a 64th of what the memory limit leaves the arena, or of the free
// device memory, at most 1 GiB (the scratch table of DESIGN.md section 31: up to 48 bytes per text byte when every op is two bytes).
uint64_t swg_ucsc_default_batch(swg_ctx* ctx) {
  size_t room = swg_arena_budget(ctx);
  if (!ctx->mem_limit) {
    size_t free_b = 0, total_b = 0;
    room = hipSetDevice(ctx->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess ? free_b + ctx->arena_cap : size_t(1) << 30;
  }
  return std::max<uint64_t>(std::min<uint64_t>(room / 64, uint64_t(1) << 30), 1);
}

extern "C" int swg_ucsc_chain_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status, const swg_cigar_set* cigars,
                                      swg_ucsc_request* req) {
  return swg_ucsc_run(ctx, rec, false, seq_len, status, cigars, req);
}
extern "C" int swg_ucsc_chain_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status,
                                             const swg_cigar_set* cigars, swg_ucsc_request* req) {
  return swg_ucsc_run(ctx, rec, true, seq_len, status, cigars, req);
}
