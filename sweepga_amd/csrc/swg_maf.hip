// Alignment blocks with their gapped bases: every usable entry cut at its breakers into blocks, and for each
// block the two rows of bases with their gaps -- what a MAF `s` line holds.  The parse, the four prefix sums, op_first[] and the entry
// states are cigar_build's, the usable test and the 32-bit base loads swg_seq_usable.h's; include/sweepga_gpu.h states the
// definitions, swg_maf_walk.h holds the rules.  An op's part in the rows follows from its advances alone, so no letter is read again.
//
//   maf_entries   one thread per entry: usable or not, the ids checked, empty / no_sequence / out_of_sequence into the scalars.
//   maf_ops       one thread per op, entries found as eqx_ops finds them: the op's alignment columns (0 for a breaker and outside
//                 the usable entries) and its breaker flag into two u64 arrays, a candidate-start flag (a non-breaker whose predecessor
//                 is a breaker or another entry), the bases under breakers summed per work-group.
//   (scans)       G[]: the alignment columns in front of every op; BK[]: the breakers in front of every op.
//   (compaction)  swg_flags_count / swg_flags_compact over the start flags: the candidates, ascending.
//   maf_runs      one thread per candidate: its entry by search, its end from the next start and BK[] (no loop), its row and its
//                 plan from X, Y, A, G at both ends; keep flag aligned > 0; gap_only, columns and aligned summed per wavefront.
//   (compaction)  the kept candidates, ascending: the blocks.
//   maf_gather    one thread per block: row and plan to their place, 2 * columns into the scan's array.
//   (scan)        64-bit inclusive sums: where each block's text ends, and the text's length.
//   maf_first     one thread per block: text_first.
//   maf_text      the hot kernel: the output in tiles of SWG_MAF_TEXT_TILE bytes, one work-group each.  Two searches in the ends give
//                 the blocks the tile touches, their ends go to LDS, and every output position finds its block there, its row and its
//                 alignment column; its op by a search in G[] between the block's ops -- once per wavefront; the 64 op borders from
//                 there on are loaded one per lane, and a lane whose columns lie behind the wavefront's op finds its own op by a
//                 search along the lanes, in memory only beyond them.  Four consecutive output bytes per lane: inside one op and one row the
//                 source is one or two aligned 32-bit loads (on '-' byte-swapped and sent through comp_raw, which sits in LDS), a
//                 gap is a constant, and the four bytes leave as one dword store.
//
// No work-group waits for another inside a launch; no atomics in the text kernel; the result does not depend on the grid's shape.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_cigar_build.h"
#include "swg_seq_usable.h"
#include "swg_maf_walk.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;  // TB, WAVES, wave_sum, reserve_first
using swg_lift_ix::LiftCols;
using namespace swg_cigar;
using namespace swg_seq_usable;
using namespace swg_maf;

static_assert(sizeof(swg_maf_block) == 64 && sizeof(swg_maf_request) == 152 && sizeof(swg_maf_options) == 24 && sizeof(swg_maf_counts) == 128,
              "include/sweepga_gpu.h states these sizes");
enum { F_USABLE = C_BUILD_TOTAL, F_EMPTY, F_BAD_ID, F_NO_SEQ, F_OUT_SEQ, F_BAD_OFFSET, F_SKIP_T, F_SKIP_Q, F_CANDIDATES, F_BLOCKS, F_GAP_ONLY, F_COLUMNS,
       F_ALIGNED, F_TOTAL };

constexpr int TILE = (int)SWG_MAF_TEXT_TILE;
constexpr int MAX_SLOTS = TILE / 2 + 2;  // a block's text has two bytes or more: at most TILE / 2 + 1 blocks touch a tile
static_assert(TB == 256 && WAVES == 4 && TILE % (4 * TB) == 0, "whole rounds of the work-group per tile");

__device__ const uint8_t d_comp_raw[256] = SWG_MAF_COMP_RAW;

unsigned grid_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

__global__ __launch_bounds__(TB) void maf_offsets_kernel(const uint64_t* __restrict__ offset, uint32_t n_seq, unsigned long long* __restrict__ scalars) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (offsets_descend(offset, n_seq, s)) atomicOr(&scalars[F_BAD_OFFSET], 1ull);
}

__global__ __launch_bounds__(TB) void maf_entries_kernel(CigarSet S, LiftCols c, uint32_t n_seq, uint32_t set, const uint64_t* __restrict__ seq_off,
                                                         uint8_t* __restrict__ usable, unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  Usable u{false, false, false, false, false};
  if (j < S.k) {
    u = usable_of(S, c, n_seq, set, seq_off, j);
    usable[j] = u.ok ? 1 : 0;
  }
  count_votes(u.ok, &scalars[F_USABLE]);
  count_votes(u.empty, &scalars[F_EMPTY]);
  count_votes(u.no_seq, &scalars[F_NO_SEQ]);
  count_votes(u.out_seq, &scalars[F_OUT_SEQ]);
  if (__ballot(u.bad_id) && (threadIdx.x & 63) == 0) atomicOr(&scalars[F_BAD_ID], 1ull);
}

struct OpArrays {
  uint64_t* G;     // [ops + 1] the alignment columns, then their exclusive sums
  uint64_t* BK;    // [ops + 1] the breaker flags, then their exclusive sums
  uint8_t* start;  // [ops] the op starts a candidate
};

__global__ __launch_bounds__(TB) void maf_ops_kernel(CigarSet S, OpArrays A, uint32_t g, const uint8_t* __restrict__ usable,
                                                     unsigned long long* __restrict__ scalars) {
  __shared__ uint32_t l_range[2];
  __shared__ unsigned long long l_skip[2][WAVES];
  const uint64_t tile0 = (uint64_t)blockIdx.x * TB;  // (the grid covers the ops: tile0 < S.ops)
  if (threadIdx.x < 2) {
    const uint64_t edge = threadIdx.x == 0 ? tile0 : (tile0 + TB - 1 < S.ops ? tile0 + TB - 1 : S.ops - 1);
    l_range[threadIdx.x] = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), (uint32_t)edge);
  }
  __syncthreads();
  const uint64_t r = tile0 + threadIdx.x;
  unsigned long long skip_t = 0, skip_q = 0;
  if (r < S.ops) {
    const uint32_t e = entry_at(S.op_first, l_range[0], l_range[1], (uint32_t)r);
    uint64_t cols = 0, breaker = 0;
    uint8_t start = 0;
    if (usable[e]) {
      const uint64_t dx = S.P.X[r + 1] - S.P.X[r], dy = S.P.Y[r + 1] - S.P.Y[r];
      if (is_breaker(dx, dy, g)) {
        breaker = 1, skip_t = dy, skip_q = dx;
      } else {
        cols = op_columns(dx, dy);
        start = r == S.op_first[e] || op_is_breaker(S.P, r - 1, g) ? 1 : 0;
      }
    }
    A.G[r + 1] = cols;  // (G[0], BK[0] are the host's 0: the inclusive scans leave the exclusive sums)
    A.BK[r + 1] = breaker;
    A.start[r] = start;
  }
  // folded along the wavefront, then across the work-group: one pair of atomics per work-group that met a breaker
  skip_t = wave_sum(skip_t), skip_q = wave_sum(skip_q);
  if ((threadIdx.x & 63) == 0) l_skip[0][threadIdx.x >> 6] = skip_t, l_skip[1][threadIdx.x >> 6] = skip_q;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) sum += l_skip[threadIdx.x][w];
    if (sum) atomicAdd(&scalars[threadIdx.x == 0 ? F_SKIP_T : F_SKIP_Q], sum);
  }
}

struct Plan {  // what maf_text needs of a block
  uint64_t tb, qb;  // the target byte of op r, column d is bases[tb + Y[r] + d]; the query byte bases[qb + X[r] + d], on '-' bases[qb - X[r] - d]
  uint64_t G0;      // the alignment columns in front of the block
  uint32_t op_first, op_end;  // over the whole call's ops
  uint32_t columns, minus;
};
static_assert(sizeof(Plan) == 40, "stated in include/sweepga_gpu.h's scratch account");

struct Runs {
  uint64_t n;            // candidates, or blocks
  const uint32_t* list;  // [n] the candidates' first ops, ascending; or the kept candidates
  swg_maf_block* row;    // [n]
  Plan* plan;            // [n]
  uint8_t* keep;         // [n] (candidates)
  uint64_t* text_end;    // [n] (blocks) 2 * columns, then their inclusive sums
};

__global__ __launch_bounds__(TB) void maf_runs_kernel(CigarSet S, LiftCols c, Seqs seqs, OpArrays A, Runs R, unsigned long long* __restrict__ scalars) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  unsigned long long gap_only = 0, columns = 0, aligned = 0;
  if (i < R.n) {
    const uint32_t start = R.list[i];
    const uint32_t e = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), start);
    const uint32_t first = S.op_first[e], op_end = S.op_first[e + 1];
    uint32_t next = op_end;
    if (i + 1 < R.n) {
      const uint32_t n2 = R.list[i + 1];
      if (n2 < op_end) next = n2;
    }
    const uint32_t end = (uint32_t)candidate_end(next, A.BK[next], A.BK[start]);
    const uint32_t rec = S.record[e];
    const bool minus = c.strand[rec] != 0;
    const uint32_t q_start = c.start[0][rec], q_end = c.end[0][rec], t_start = c.start[1][rec];
    uint32_t w[10];
    block_words(S.P, first, start, end, minus, q_start, q_end, t_start, w);
    const bool keep = w[6] != 0;
    R.keep[i] = keep ? 1 : 0;
    if (keep) {
      uint4* o = reinterpret_cast<uint4*>(R.row + i);  // 64 bytes: four 16-byte stores (arena blocks are 16-byte aligned)
      o[0] = make_uint4(rec, e, w[0], w[1]);
      o[1] = make_uint4(w[2], w[3], w[4], w[5]);
      o[2] = make_uint4(w[6], w[7], w[8], w[9]);
      o[3] = make_uint4(0u, 0u, 0u, 0u);
      Plan p;
      p.tb = seqs.offset[c.id[1][rec]] + t_start - S.P.Y[first];  // (modulo 2^64: the sum with Y[r] is an index into the bases)
      const uint64_t q0 = seqs.offset[c.id[0][rec]];
      p.qb = minus ? q0 + q_end - 1 + S.P.X[first] : q0 + q_start - S.P.X[first];
      p.G0 = A.G[start];
      p.op_first = start, p.op_end = end;
      p.columns = w[7], p.minus = minus ? 1u : 0u;
      R.plan[i] = p;
      columns = w[7], aligned = w[6];
    } else {
      gap_only = 1;
    }
  }
  gap_only = wave_sum(gap_only), columns = wave_sum(columns), aligned = wave_sum(aligned);
  if ((threadIdx.x & 63) == 0) {
    if (gap_only) atomicAdd(&scalars[F_GAP_ONLY], gap_only);
    if (columns) atomicAdd(&scalars[F_COLUMNS], columns);
    if (aligned) atomicAdd(&scalars[F_ALIGNED], aligned);
  }
}

__global__ __launch_bounds__(TB) void maf_gather_kernel(Runs R, Runs O) {
  const uint64_t b = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (b >= O.n) return;
  const uint32_t i = O.list[b];
  const uint4* in = reinterpret_cast<const uint4*>(R.row + i);
  uint4* o = reinterpret_cast<uint4*>(O.row + b);
  const uint4 w0 = in[0], w1 = in[1], w2 = in[2], w3 = in[3];
  o[0] = w0, o[1] = w1, o[2] = w2, o[3] = w3;
  O.plan[b] = R.plan[i];
  O.text_end[b] = 2ull * w2.y;  // columns
}

__global__ __launch_bounds__(TB) void maf_first_kernel(Runs O) {
  const uint64_t b = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (b >= O.n) return;
  O.row[b].text_first = O.text_end[b] - 2ull * O.row[b].columns;
}

// the first block in [0, n) whose text ends behind byte o (there is one)
__device__ __forceinline__ uint64_t block_at(const uint64_t* __restrict__ text_end, uint64_t n, uint64_t o) {
  uint64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (text_end[mid] > o) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
// the last op r in [lo, hi] with G[r] <= s (G[lo] <= s < G[hi + 1]): the op that alignment column s belongs to
__device__ __forceinline__ uint32_t op_at(const uint64_t* __restrict__ G, uint32_t lo, uint32_t hi, uint64_t s) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (G[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct ColOp {       // what a lane knows of the op its columns lie in
  uint64_t g0, g1;   // the op's alignment columns
  OpBytes at;
  uint32_t r;
};
// op r of the block of plan p
__device__ __forceinline__ ColOp op_of(const Prefix& P, const uint64_t* __restrict__ G, const Plan& p, uint32_t r) {
  ColOp o;
  o.r = r;
  o.g0 = G[r], o.g1 = G[r + 1];
  const uint64_t x0 = P.X[r], y0 = P.Y[r];
  o.at.rows = op_rows(P.X[r + 1] - x0, P.Y[r + 1] - y0);
  o.at.minus = p.minus;
  o.at.t_at = p.tb + y0;
  o.at.q_at = p.minus ? p.qb - x0 : p.qb + x0;
  return o;
}
__device__ __forceinline__ ColOp locate(const Prefix& P, const uint64_t* __restrict__ G, const Plan& p, uint64_t col) {
  return op_of(P, G, p, op_at(G, p.op_first, p.op_end - 1, col));
}

constexpr uint32_t DASH4 = 0x2d2d2d2du;

// W output bytes per lane and store: 1, or 4 packed into one dword
template <int W>
__global__ __launch_bounds__(TB) void maf_text_kernel(Prefix P, const uint64_t* __restrict__ G, Runs O, Seqs seqs, uint64_t text_bytes, char* __restrict__ out) {
  __shared__ uint32_t l_end[MAX_SLOTS];  // where the tile's blocks end, relative to the tile (the last one clamped to TILE)
  __shared__ uint64_t l_span[2];
  __shared__ uint8_t l_comp[256];
  const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;
  const uint32_t len = text_bytes - tile0 < (uint64_t)TILE ? (uint32_t)(text_bytes - tile0) : (uint32_t)TILE;
  l_comp[threadIdx.x] = d_comp_raw[threadIdx.x];
  if (threadIdx.x == 0) l_span[0] = block_at(O.text_end, O.n, tile0);
  if (threadIdx.x == 64) l_span[1] = block_at(O.text_end, O.n, tile0 + len - 1);
  __syncthreads();
  const uint64_t bf = l_span[0];
  uint32_t cnt = (uint32_t)(l_span[1] - bf) + 1u;
  if (cnt > (uint32_t)MAX_SLOTS) cnt = MAX_SLOTS;  // (never: every block has two bytes or more)
  for (uint32_t s = threadIdx.x; s < cnt; s += TB) {
    const uint64_t e = O.text_end[bf + s] - tile0;
    l_end[s] = e < (uint64_t)TILE ? (uint32_t)e : (uint32_t)TILE;
  }
  __syncthreads();
  const uint64_t first0 = bf ? O.text_end[bf - 1] : 0;  // where block bf begins: at or in front of the tile
#pragma unroll 1
  for (uint32_t base = 0; base < len; base += TB * W) {
    // the wavefront's first position: one search for all its lanes (every lane the same addresses)
    const uint32_t woff = base + (threadIdx.x & ~63u) * W;
    if (woff >= len) break;  // (wavefront-uniform)
    uint32_t wslot;
    {
      uint32_t lo = 0, hi = cnt - 1;  // the first slot that ends behind woff
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (l_end[mid] > woff) hi = mid;
        else lo = mid + 1;
      }
      wslot = lo;
    }
    const Plan wplan = O.plan[bf + wslot];
    const uint64_t wrel = wslot ? woff - l_end[wslot - 1] : tile0 + woff - first0;
    const ColOp wop = locate(P, G, wplan, wplan.G0 + (wrel >= wplan.columns ? wrel - wplan.columns : wrel));
    // the 64 op borders from the wavefront's op on, one per lane, ascending: one coalesced load, and a lane whose columns lie behind
    // the wavefront's op in the same block finds its op by a search along the lanes instead of one in memory
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wr = wop.r + lane < wplan.op_end ? wop.r + lane : wplan.op_end;
    const uint64_t wg = G[wr];  // (G[op_end] = the block's end: behind every column of the block)

    uint32_t off0 = base + threadIdx.x * W;
    const bool live = off0 < len;
    if (!live) off0 = woff;  // (goes along: the search along the lanes is the whole wavefront's)
    uint32_t slot = wslot;
    if (off0 >= l_end[wslot]) {
      uint32_t lo = wslot + 1, hi = cnt - 1;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (l_end[mid] > off0) hi = mid;
        else lo = mid + 1;
      }
      slot = lo;
    }
    Plan p = slot == wslot ? wplan : O.plan[bf + slot];
    uint64_t rel = slot ? off0 - l_end[slot - 1] : tile0 + off0 - first0;
    uint32_t row = rel >= p.columns ? 1u : 0u;
    uint64_t col = p.G0 + (row ? rel - p.columns : rel);
    uint32_t near = 0;  // the last lane whose border is at or below col (lane 0 holds wop.g0)
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1) {
      const uint64_t g = __shfl(wg, (int)(near + step));
      if (g <= col) near += step;
    }
    if (!live) continue;
    ColOp o = wop;
    if (slot != wslot || col < o.g0) o = locate(P, G, p, col);
    else if (col >= o.g1) o = near < 63u ? op_of(P, G, p, wop.r + near) : locate(P, G, p, col);  // (lane 63's border may not be the last one below col)
    uint32_t packed;
    if (W == 4 && off0 + 4 <= l_end[slot] && (rel + 4 <= p.columns || row) && col + 4 <= o.g1) {  // one block, one row, one op
      const uint64_t d = col - o.g0;
      if (row == 0) {
        packed = o.at.rows & ROW_T ? load_quad(seqs, o.at.t_at + d) : DASH4;
      } else if (!(o.at.rows & ROW_Q)) {
        packed = DASH4;
      } else if (!p.minus) {
        packed = load_quad(seqs, o.at.q_at + d);
      } else {
        const uint32_t q = load_quad(seqs, o.at.q_at - d - 3);  // the four bytes descend: the last one first
        packed = (uint32_t)l_comp[q >> 24] | (uint32_t)l_comp[q >> 16 & 255u] << 8 | (uint32_t)l_comp[q >> 8 & 255u] << 16 | (uint32_t)l_comp[q & 255u] << 24;
      }
    } else {
      packed = 0;
#pragma unroll 1
      for (int w = 0; w < W; ++w) {
        const uint32_t off = off0 + w;
        if (off >= len) break;
        if (w) {
          ++rel, ++col;
          if (off >= l_end[slot]) {  // the next block (every block in the tile's span has bytes)
            ++slot;
            p = O.plan[bf + slot];
            rel = 0, row = 0, col = p.G0;
          } else if (!row && rel >= p.columns) {  // the query row: the block's columns again
            row = 1, col = p.G0;
          }
          if (col < o.g0 || col >= o.g1 || rel == 0) o = locate(P, G, p, col);
        }
        const uint32_t v = row_byte(o.at, seqs.bases, l_comp, row, col - o.g0);
        if (W == 1) out[tile0 + off] = (char)v;
        else packed |= v << (8 * w);
      }
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

// bytes per lane and store of maf_text: 4 unless the environment asks for the byte form (tools/maf_bench.py measures both)
int text_form() {
  const char* e = std::getenv("SWG_MAF_TEXT_FORM");
  return e && e[0] == '1' && !e[1] ? 1 : 4;
}

// where: 0 = everything on the host, 1 = everything on the device, 2 = the host's, but seqs->bases in device memory
int maf_run(swg_ctx* ctx, const swg_records* rec, int where, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
            swg_maf_request* req) {
  const bool on_device = where == 1;
  static const char* const who = "maf_records";
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL records or request", who);
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (req->set == SWG_IV_KEPT && !status) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  const uint64_t n = rec->n, k = cigars ? cigars->k : 0;
  const uint32_t n_seq = rec->n_seq;
  uint64_t B = 0;
  SWG_TRY(cigar_set_check_host(ctx, who, cigars, on_device, n, &B));
  if (B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
  if (k && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL column", who);
  if (k && (!seqs || !seqs->offset || !seqs->bases)) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL sequences, offsets or bases", who);
  if (k && (seqs->n_seq != n_seq || seqs->reserved != 0))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the sequence set must have rec->n_seq sequences and reserved 0", who);
  uint64_t n_bases = 0;
  if (k && !on_device) {
    for (uint32_t s = 0; s < n_seq; ++s)
      if (seqs->offset[s + 1] < seqs->offset[s]) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the sequence offsets descend at sequence %u", who, s);
    n_bases = seqs->offset[n_seq];
  }
  req->ops = req->cigar_bad = req->empty = req->usable = req->no_sequence = req->out_of_sequence = 0;
  req->n_blocks = req->gap_only = req->breakers = req->skipped_t = req->skipped_q = req->columns = req->aligned = req->text_bytes = 0;
  if (!k) return SWG_OK;  // no device work
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)(on_device ? 0 : n * 26 + (size_t)n_seq * 8 + (where == 0 ? n_bases : 0)) + (size_t)B * 32 + (size_t)k * 16 + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    hipStream_t st = ctx->stream;
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    Seqs Q{seqs->offset, seqs->bases, n_bases};
    CigarSet S{};
    S.k = k, S.B = B;
    S.record = cigars->record, S.offset = cigars->offset, S.text = cigars->text;
    if (!on_device) {
      swg_stager s(ctx);
      for (int a = 0; a < 2; ++a) s.add(&c.id[a], n), s.add(&c.start[a], n), s.add(&c.end[a], n);
      s.add(&c.strand, n);
      s.add(&c.status, n);
      s.add(&S.record, k);
      s.add(&S.offset, k + 1);
      s.add(&S.text, B);
      s.add(&Q.offset, (size_t)n_seq + 1);
      if (where == 0) s.add(&Q.bases, n_bases);
      SWG_TRY(s.run());
    }
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, F_TOTAL);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(scalars, 0, F_TOTAL * sizeof(unsigned long long), st));
    uint64_t* const d_scalars = reinterpret_cast<uint64_t*>(scalars);
    if (on_device) {
      SWG_TRY(cigar_set_check_device(ctx, who, n, &S, scalars));
      if (S.B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
      if (n_seq) {  // before anything reads a base through the offsets
        SWG_LAUNCH(ctx, "maf_offsets", maf_offsets_kernel<<<grid_of(n_seq), TB, 0, st>>>(Q.offset, n_seq, scalars));
        SWG_KERNEL_CHECK(ctx);
        uint64_t bad_offset = 0;
        SWG_TRY(swg_read_scalars(ctx, d_scalars + F_BAD_OFFSET, &bad_offset, 1));
        if (bad_offset) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the sequence offsets descend", who);
      }
      SWG_TRY(swg_read_scalars(ctx, Q.offset + n_seq, &Q.n_bases, 1));
    }
    SWG_TRY(cigar_build(ctx, who, c, &S, scalars));
    const uint64_t ops = S.ops;
    OpArrays A{};
    A.G = swg_alloc<uint64_t>(ctx, ops + 1);
    A.BK = swg_alloc<uint64_t>(ctx, ops + 1);
    A.start = swg_alloc<uint8_t>(ctx, ops + 1);
    uint8_t* usable = swg_alloc<uint8_t>(ctx, k);
    SWG_CHECK_ARENA(ctx);
    SWG_LAUNCH(ctx, "maf_entries", maf_entries_kernel<<<grid_of(k), TB, 0, st>>>(S, c, n_seq, req->set, Q.offset, usable, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_HIP(ctx, hipMemsetAsync(A.G, 0, sizeof(uint64_t), st));
    SWG_HIP(ctx, hipMemsetAsync(A.BK, 0, sizeof(uint64_t), st));
    uint64_t all_columns = 0, breakers = 0, n_cand = 0, n_blocks = 0, text_bytes = 0;
    swg_flag_scan fs{};
    if (ops) {
      SWG_LAUNCH_N(ctx, "maf_ops", ops, maf_ops_kernel<<<grid_of(ops), TB, 0, st>>>(S, A, req->split_gap, usable, scalars));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, A.G, A.G, ops + 1));
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, A.BK, A.BK, ops + 1));
      SWG_TRY(swg_flags_count(ctx, A.start, ops, &fs, d_scalars + F_CANDIDATES));
      SWG_TRY(swg_read_scalars(ctx, A.G + ops, &all_columns, 1));
      SWG_TRY(swg_read_scalars(ctx, A.BK + ops, &breakers, 1));
    }
    uint64_t h[F_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, d_scalars, h, F_TOTAL));
    if (h[F_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: a record of the set has a sequence id >= n_seq", who);
    if (all_columns >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 alignment columns or more in one call (of all candidates, those of gaps only included)", who);
    n_cand = h[F_CANDIDATES];
    Runs O{};
    if (n_cand) {
      Runs R{};
      R.n = n_cand;
      uint32_t* list = swg_alloc<uint32_t>(ctx, n_cand);
      R.row = swg_alloc<swg_maf_block>(ctx, n_cand);
      R.plan = swg_alloc<Plan>(ctx, n_cand);
      R.keep = swg_alloc<uint8_t>(ctx, n_cand);
      SWG_CHECK_ARENA(ctx);
      SWG_TRY(swg_flags_compact(ctx, fs, list));
      R.list = list;
      SWG_LAUNCH_N(ctx, "maf_runs", n_cand, maf_runs_kernel<<<grid_of(n_cand), TB, 0, st>>>(S, c, Q, A, R, scalars));
      SWG_KERNEL_CHECK(ctx);
      swg_flag_scan ks{};
      SWG_TRY(swg_flags_count(ctx, R.keep, n_cand, &ks, d_scalars + F_BLOCKS));
      SWG_TRY(swg_read_scalars(ctx, d_scalars + F_BLOCKS, &n_blocks, 1));
      if (n_blocks) {
        O.n = n_blocks;
        uint32_t* kept = swg_alloc<uint32_t>(ctx, n_blocks);
        O.row = swg_alloc<swg_maf_block>(ctx, n_blocks);
        O.plan = swg_alloc<Plan>(ctx, n_blocks);
        O.text_end = swg_alloc<uint64_t>(ctx, n_blocks);
        SWG_CHECK_ARENA(ctx);
        SWG_TRY(swg_flags_compact(ctx, ks, kept));
        O.list = kept;
        SWG_LAUNCH_N(ctx, "maf_gather", n_blocks, maf_gather_kernel<<<grid_of(n_blocks), TB, 0, st>>>(R, O));
        SWG_KERNEL_CHECK(ctx);
        SWG_TRY(swg_inclusive_sum_scan_u64(ctx, O.text_end, O.text_end, n_blocks));
        SWG_TRY(swg_read_scalars(ctx, O.text_end + (n_blocks - 1), &text_bytes, 1));
        SWG_LAUNCH_N(ctx, "maf_first", n_blocks, maf_first_kernel<<<grid_of(n_blocks), TB, 0, st>>>(O));
        SWG_KERNEL_CHECK(ctx);
        if (req->text && text_bytes <= req->text_capacity) {
          char* out = swg_alloc<char>(ctx, text_bytes);
          SWG_CHECK_ARENA(ctx);
          const unsigned tiles = (unsigned)((text_bytes + TILE - 1) / TILE);
          if (text_form() == 1) SWG_LAUNCH_N(ctx, "maf_text", text_bytes, maf_text_kernel<1><<<tiles, TB, 0, st>>>(S.P, A.G, O, Q, text_bytes, out));
          else SWG_LAUNCH_N(ctx, "maf_text", text_bytes, maf_text_kernel<4><<<tiles, TB, 0, st>>>(S.P, A.G, O, Q, text_bytes, out));
          SWG_KERNEL_CHECK(ctx);
          SWG_HIP(ctx, hipMemcpyAsync(req->text, out, text_bytes, hipMemcpyDeviceToHost, st));
        }
        if (req->blocks && n_blocks <= req->block_capacity)
          SWG_HIP(ctx, hipMemcpyAsync(req->blocks, O.row, n_blocks * sizeof(swg_maf_block), hipMemcpyDeviceToHost, st));
      }
    }
    uint64_t f[F_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, d_scalars, f, F_TOTAL));  // (synchronises: the copies above are done)
    req->ops = ops, req->cigar_bad = f[C_BAD_ENTRIES], req->empty = f[F_EMPTY], req->usable = f[F_USABLE];
    req->no_sequence = f[F_NO_SEQ], req->out_of_sequence = f[F_OUT_SEQ];
    req->n_blocks = n_blocks, req->gap_only = f[F_GAP_ONLY], req->breakers = breakers, req->skipped_t = f[F_SKIP_T], req->skipped_q = f[F_SKIP_Q];
    req->columns = f[F_COLUMNS], req->aligned = f[F_ALIGNED], req->text_bytes = text_bytes;
    return SWG_OK;
  });
}

}  // namespace

int swg_maf_run(swg_ctx* ctx, const swg_records* rec, int where, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                swg_maf_request* req) {
  try {
    return maf_run(ctx, rec, where, status, cigars, seqs, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_maf_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                               swg_maf_request* req) {
  return swg_maf_run(ctx, rec, 0, status, cigars, seqs, req);
}
extern "C" int swg_maf_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                                      swg_maf_request* req) {
  return swg_maf_run(ctx, rec, 1, status, cigars, seqs, req);
}
