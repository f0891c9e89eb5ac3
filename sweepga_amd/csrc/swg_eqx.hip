// Resolved CIGARs: every usable entry rewritten in canonical =/X form against the sequences -- the columns of
// each run of M, = and X ops compared base by base and run-length encoded, every other op copied -- with exact matches, mismatches
// and block length per entry.  The parse, the four prefix sums, op_first[] and the entry states are cigar_build's, the kind bytes
// letters_of_chunk's; include/sweepga_gpu.h states the definitions, swg_eqx_walk.h holds the rules.
//
//   eqx_letters    one thread per 16 text bytes: the kind byte of every op (swg_diffs_letters.h) and the byte position of its letter.
//   eqx_entries    one thread per entry: usable or not, the ids checked, empty / no_sequence / out_of_sequence into the scalars, the
//                  entry's row cleared but for its record.
//   eqx_ops        one thread per op, entries found as variants_ops finds them: the op's COLUMNS into a u64 array (a column op of a
//                  usable entry, else 0), 1 into a second one for every other op of a usable entry (a VERBATIM item), and a class
//                  byte: M / = / X, whether the op holds the first column of its run, whether it is the first op of its entry.  The
//                  bases under N ops go to the entry's row.
//   (scans)        C[]: the columns of all runs numbered consecutively, in (entry, op, column) order; NC[]: the verbatim items in
//                  front of every op.
//   eqx_columns    the hot kernel: a tile of SWG_EQX_COLUMN_TILE columns per work-group, four consecutive columns per lane and round.
//                  A wavefront searches the op of its first column once; a lane whose four columns lie in that op takes the target's
//                  and the query's four bytes as one or two 32-bit loads each (on '-' the query's descend and are complemented), any
//                  other lane searches per column and loads bytes.  eq and the run-first bit of every column go to LDS, a nibble each
//                  per lane; after one barrier a column is a BOUNDARY when it is the first of its run or its eq differs from the
//                  previous column's (the tile's first column has the one in front of the tile computed for it), and its byte is
//                  written: 0, or 1 | eq << 1 -- the one byte of scratch a column gets, flag and letter at once, so nothing is
//                  recomputed later.  The six sums stay in the lane while its columns stay in one entry, runs of one entry are
//                  folded along the wavefront, and the run's first lane adds them to the entry's row.
//   (compaction)   swg_flags_count / swg_flags_compact over the bytes: the boundaries, ascending, are the GENERATED ops; each one's
//                  length is the next one's column minus its own, the total as sentinel.
//   eqx_generated  one thread per generated op: its op by a search in C[], item NC[op] + rank, `<length><letter>` and its byte length.
//   eqx_verbatim   one thread per op: a verbatim op i is item NC[i] + (boundaries below C[i]), its bytes are the text from behind the
//                  previous letter up to its own.
//   (scan)         64-bit inclusive sums of the item lengths: where every item's bytes go, and the text's length.
//   eqx_finish     one thread per entry: its items from NC[] and the boundary rank at its first and last op, out_ops, text_first,
//                  text_len, inserted, deleted, block, CHANGED (from the sums: see DESIGN.md), and the totals into the scalars.
//   eqx_text       a tile of SWG_EQX_TEXT_TILE output bytes per work-group: two searches give the items that touch it, every item
//                  (at most 11 bytes) is formatted or copied into LDS by one lane, and the tile streams out as consecutive dwords.
//
// No work-group waits for another inside a launch; integer atomics only; the result does not depend on the grid's shape.
#include <algorithm>
#include <cstring>
#include <new>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_cigar_build.h"
#include "swg_diffs_walk.h"
#include "swg_diffs_letters.h"
#include "swg_eqx_walk.h"
#include "swg_seq_usable.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;  // TB, WAVES, EMPTY, run_end, run_sum, wave_sum, reserve_first
using swg_lift_ix::LiftCols;
using namespace swg_cigar;
using namespace swg_diffs;
using namespace swg_eqx;
using namespace swg_seq_usable;  // Seqs, count_votes, offsets_descend, usable_of, entry_at, load_quad

static_assert(sizeof(swg_eqx_entry) == 64 && sizeof(swg_eqx_request) == 168 && sizeof(swg_eqx_options) == 24 && sizeof(swg_eqx_counts) == 128,
              "include/sweepga_gpu.h states these sizes");
enum { F_USABLE = C_BUILD_TOTAL, F_EMPTY, F_BAD_ID, F_NO_SEQ, F_OUT_SEQ, F_BAD_OFFSET, F_GENERATED, F_CHANGED, F_SUMS, F_TOTAL = F_SUMS + 6 };
// the class byte of an op: bits 0 .. 1 the column class of a usable entry's column op, then
enum : uint32_t { B_RUN_FIRST = 4, B_VERBATIM = 8, B_ENTRY_FIRST = 16 };

constexpr int CTILE = (int)SWG_EQX_COLUMN_TILE, QUADS = CTILE / 4, ROUNDS = QUADS / TB;
constexpr int TTILE = (int)SWG_EQX_TEXT_TILE;
static_assert(TB == 256 && CTILE % (4 * TB) == 0 && TTILE % 4 == 0, "whole rounds of the work-group per tile");
static_assert(CTILE / TB * 64 < (1 << SUM_BITS), "a wavefront's columns of one tile fit a field of the packed sums");

unsigned grid_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

__global__ __launch_bounds__(TB) void eqx_offsets_kernel(const uint64_t* __restrict__ offset, uint32_t n_seq, unsigned long long* __restrict__ scalars) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (offsets_descend(offset, n_seq, s)) atomicOr(&scalars[F_BAD_OFFSET], 1ull);
}

__global__ __launch_bounds__(TB) void eqx_letters_kernel(CigarSet S, int aligned, uint8_t* __restrict__ kind, uint32_t* __restrict__ pos) {
  const uint64_t chunk = (uint64_t)blockIdx.x * TB + threadIdx.x, p0 = chunk * 16;
  letters_of_chunk(S, aligned, chunk, kind);
  if (p0 >= S.B) return;
  uint64_t r = S.chunk_rank[chunk];
  const uint64_t p1 = p0 + 16 < S.B ? p0 + 16 : S.B;
  for (uint64_t p = p0; p < p1; ++p) {
    if (is_digit((unsigned char)S.text[p])) continue;
    if (r < S.ops) pos[r] = (uint32_t)p;  // (always: the ranks are the parse's own count of these bytes; B < 2^32)
    ++r;
  }
}

__global__ __launch_bounds__(TB) void eqx_entries_kernel(CigarSet S, LiftCols c, uint32_t n_seq, uint32_t set, const uint64_t* __restrict__ seq_off,
                                                         uint8_t* __restrict__ usable, swg_eqx_entry* __restrict__ entries,
                                                         unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  bool ok = false, empty = false, bad_id = false, no_seq = false, out_seq = false;
  if (j < S.k) {
    const uint32_t rec = S.record[j];
    const Usable u = usable_of(S, c, n_seq, set, seq_off, j);
    ok = u.ok, empty = u.empty, bad_id = u.bad_id, no_seq = u.no_seq, out_seq = u.out_seq;
    usable[j] = ok ? 1 : 0;
    uint4* o = reinterpret_cast<uint4*>(entries + j);  // 64 bytes: four 16-byte stores (arena blocks are 16-byte aligned)
    o[0] = make_uint4(rec, 0u, 0u, 0u);
    o[1] = o[2] = o[3] = make_uint4(0u, 0u, 0u, 0u);
  }
  count_votes(ok, &scalars[F_USABLE]);
  count_votes(empty, &scalars[F_EMPTY]);
  count_votes(no_seq, &scalars[F_NO_SEQ]);
  count_votes(out_seq, &scalars[F_OUT_SEQ]);
  if (__ballot(bad_id) && (threadIdx.x & 63) == 0) atomicOr(&scalars[F_BAD_ID], 1ull);
}

// the last op r in [lo, hi] with C[r] <= s (C[lo] <= s, hi < ops, s < C[ops]): the op that column s belongs to
__device__ __forceinline__ uint32_t op_at(const uint64_t* __restrict__ C, uint32_t lo, uint32_t hi, uint64_t s) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (C[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// the entries of list[0 .. n) (ascending) below v
__device__ __forceinline__ uint32_t rank_below(const uint32_t* __restrict__ list, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (list[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the letter of op r as the text has it (the kind byte tells M and X; '=' shares its 0 with S, H and P)
__device__ __forceinline__ uint32_t class_of_op(const CigarSet& S, const uint8_t* __restrict__ kind, const uint32_t* __restrict__ pos, uint64_t r) {
  const uint32_t kd = kind[r];
  if (kd & K_M) return L_M;
  if (kd & K_SNP) return L_X;
  return kd == 0 ? column_class((unsigned char)S.text[pos[r]]) : 0u;
}

struct OpArrays {
  const uint8_t* kind;   // [ops]
  const uint32_t* pos;   // [ops] the byte of every op's letter
  uint8_t* cls;          // [ops]
  uint64_t* C;           // [ops + 1] the columns, then their exclusive sums
  uint64_t* NC;          // [ops + 1] the verbatim items, then their exclusive sums
};

__global__ __launch_bounds__(TB) void eqx_ops_kernel(CigarSet S, OpArrays A, const uint8_t* __restrict__ usable, swg_eqx_entry* __restrict__ entries) {
  __shared__ uint32_t l_range[2];
  const uint64_t tile0 = (uint64_t)blockIdx.x * TB;  // (the grid covers the ops: tile0 < S.ops)
  if (threadIdx.x < 2) {
    const uint64_t edge = threadIdx.x == 0 ? tile0 : (tile0 + TB - 1 < S.ops ? tile0 + TB - 1 : S.ops - 1);
    l_range[threadIdx.x] = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), (uint32_t)edge);
  }
  __syncthreads();
  const uint64_t r = tile0 + threadIdx.x;
  if (r >= S.ops) return;
  const uint32_t e = entry_at(S.op_first, l_range[0], l_range[1], (uint32_t)r);
  const uint32_t first = S.op_first[e];
  uint32_t b = r == first ? B_ENTRY_FIRST : 0u;
  uint64_t cols = 0, verbatim = 0;
  if (usable[e]) {
    const uint32_t cl = class_of_op(S, A.kind, A.pos, r);
    if (cl) {
      cols = S.P.A[r + 1] - S.P.A[r];
      b |= cl;
      if (cols) {  // the first column of its run when every column op between the run's start and here is empty
        bool run_first = true;
        for (uint64_t q = r; q > first; --q) {
          if (!class_of_op(S, A.kind, A.pos, q - 1)) break;
          if (S.P.A[q] - S.P.A[q - 1]) {
            run_first = false;
            break;
          }
        }
        if (run_first) b |= B_RUN_FIRST;
      }
    } else {
      verbatim = 1;
      b |= B_VERBATIM;
      if (A.kind[r] & K_SKIP) {  // an N op advances the target and is no deleted base: eqx_finish takes it off
        const uint64_t l = S.P.Y[r + 1] - S.P.Y[r];
        if (l) atomicAdd(&entries[e].deleted, (uint32_t)l);
      }
    }
  }
  A.cls[r] = (uint8_t)b;
  A.C[r + 1] = cols;  // (C[0], NC[0] are the host's 0: the inclusive scans leave the exclusive sums)
  A.NC[r + 1] = verbatim;
}

// What a lane knows of the op its columns lie in.
struct ColOp {
  uint64_t c0, c1;  // the op's columns
  uint64_t t_at;    // the op's first target byte, as an index into the bases
  uint64_t q_at;    // the op's first query byte: on '-' the columns descend from it
  uint32_t e, cls, minus;
};
__device__ __forceinline__ ColOp locate(const CigarSet& S, const LiftCols& c, const Seqs& seqs, const OpArrays& A, uint32_t r_lo, uint32_t r_hi,
                                        uint32_t e_lo, uint32_t e_hi, uint64_t col) {
  ColOp o;
  const uint32_t r = op_at(A.C, r_lo, r_hi, col);
  o.c0 = A.C[r], o.c1 = A.C[r + 1];
  o.e = entry_at(S.op_first, e_lo, e_hi, r);
  o.cls = A.cls[r];
  const uint32_t first = S.op_first[o.e], rec = S.record[o.e];
  const uint64_t x = S.P.X[r] - S.P.X[first], y = S.P.Y[r] - S.P.Y[first];
  o.minus = c.strand[rec] != 0;
  o.t_at = seqs.offset[c.id[1][rec]] + c.start[1][rec] + y;
  const uint64_t q0 = seqs.offset[c.id[0][rec]];
  o.q_at = o.minus ? q0 + c.end[0][rec] - 1 - x : q0 + c.start[0][rec] + x;
  return o;
}
struct Pending {  // the sums of the entry a lane's last columns lay in
  uint32_t e;
  ColumnSums s;
};
__device__ __forceinline__ void sums_flush(swg_eqx_entry* __restrict__ entries, uint32_t e, const ColumnSums& s) {
  uint32_t* f[6] = {&entries[e].matches, &entries[e].mismatches, &entries[e].n_columns, &entries[e].eq_wrong, &entries[e].x_wrong, &entries[e].m_columns};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const uint32_t v = sums_field(s, i);
    if (v) atomicAdd(f[i], v);
  }
}
__device__ __forceinline__ void pending_take(Pending& p, swg_eqx_entry* __restrict__ entries, uint32_t e) {
  if (p.e == e) return;
  if (p.e != NONE32) sums_flush(entries, p.e, p.s);  // (an entry border inside the lane's columns)
  p.e = e, p.s.w[0] = p.s.w[1] = 0;
}

__global__ __launch_bounds__(TB) void eqx_columns_kernel(CigarSet S, LiftCols c, Seqs seqs, OpArrays A, uint64_t total, swg_eqx_entry* __restrict__ entries,
                                                         uint8_t* __restrict__ flags) {
  __shared__ uint8_t l_quad[QUADS];  // per four columns: eq in bits 0 .. 3, first-of-its-run in bits 4 .. 7
  __shared__ uint32_t l_op[2], l_entry[2], l_prev;
  const uint64_t tile0 = (uint64_t)blockIdx.x * CTILE;  // (the grid covers the columns: tile0 < total)
  if (threadIdx.x < 2) {
    const uint64_t edge = threadIdx.x == 0 ? tile0 : (tile0 + CTILE - 1 < total ? tile0 + CTILE - 1 : total - 1);
    const uint32_t r = op_at(A.C, 0, (uint32_t)(S.ops - 1), edge);
    l_op[threadIdx.x] = r;
    l_entry[threadIdx.x] = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), r);
  }
  if (threadIdx.x == 64) {  // eq of the column in front of the tile
    uint32_t eq = 0;
    if (tile0) {
      const ColOp o = locate(S, c, seqs, A, 0, (uint32_t)(S.ops - 1), 0, (uint32_t)(S.k - 1), tile0 - 1);
      const uint64_t b = tile0 - 1 - o.c0;
      const uint32_t t = code_of(seqs.bases[o.t_at + b]), q = code_of(seqs.bases[o.minus ? o.q_at - b : o.q_at + b]);
      eq = column_eq(t, o.minus ? comp_code(q) : q);
    }
    l_prev = eq;
  }
  __syncthreads();
  const uint32_t r_lo = l_op[0], r_hi = l_op[1], e_lo = l_entry[0], e_hi = l_entry[1];
  Pending pend;
  pend.e = NONE32, pend.s.w[0] = pend.s.w[1] = 0;
  ColOp own;
  own.c0 = own.c1 = 0;  // (no column: the first one searches)
#pragma unroll 1
  for (int j = 0; j < ROUNDS; ++j) {
    const uint32_t quad = (uint32_t)j * TB + threadIdx.x;
    const uint64_t wave0 = tile0 + 4ull * ((uint32_t)j * TB + (threadIdx.x & ~63u));  // the wavefront's first column
    if (wave0 >= total) break;                                                      // (wavefront-uniform)
    const ColOp w = locate(S, c, seqs, A, r_lo, r_hi, e_lo, e_hi, wave0);           // (one search for the wavefront: every lane the same)
    const uint64_t col0 = tile0 + 4ull * quad;
    if (col0 >= total) continue;
    uint32_t eq4 = 0, first4 = 0;
    if (col0 >= w.c0 && col0 + 4 <= w.c1) {
      const uint64_t b = col0 - w.c0;
      const uint32_t t = load_quad(seqs, w.t_at + b);
      const uint32_t q = w.minus ? __builtin_bswap32(load_quad(seqs, w.q_at - b - 3)) : load_quad(seqs, w.q_at + b);
      pending_take(pend, entries, w.e);
      const uint32_t cl = w.cls & 3u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t r = code_of((uint8_t)(t >> (8 * i))), a0 = code_of((uint8_t)(q >> (8 * i))), a = w.minus ? comp_code(a0) : a0;
        const bool eq = column_eq(r, a);
        sums_add(pend.s, cl, eq, column_n(r, a));
        eq4 |= (eq ? 1u : 0u) << i;
      }
      first4 = b == 0 && (w.cls & B_RUN_FIRST) ? 1u : 0u;
    } else {
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
        const uint64_t col = col0 + i;
        if (col >= total) break;
        if (col < own.c0 || col >= own.c1) own = locate(S, c, seqs, A, r_lo, r_hi, e_lo, e_hi, col);
        const uint64_t b = col - own.c0;
        const uint32_t r = code_of(seqs.bases[own.t_at + b]), a0 = code_of(seqs.bases[own.minus ? own.q_at - b : own.q_at + b]);
        const uint32_t a = own.minus ? comp_code(a0) : a0;
        const bool eq = column_eq(r, a);
        pending_take(pend, entries, own.e);
        sums_add(pend.s, own.cls & 3u, eq, column_n(r, a));
        eq4 |= (eq ? 1u : 0u) << i;
        first4 |= (b == 0 && (own.cls & B_RUN_FIRST) ? 1u : 0u) << i;
      }
    }
    l_quad[quad] = (uint8_t)(eq4 | first4 << 4);
  }
  {  // runs of one entry along the wavefront: the run's first lane adds the run's sums
    const int lane = threadIdx.x & 63;
    const unsigned long long key = pend.e == NONE32 ? EMPTY : (unsigned long long)pend.e;
    if (__ballot(key != EMPTY)) {
      const unsigned long long before = __shfl_up(key, 1);
      const bool first_lane = lane == 0 || key != before;
      run_sum(pend.s.w, lane, run_end(__ballot(first_lane), lane));
      if (first_lane && key != EMPTY) sums_flush(entries, pend.e, pend.s);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < ROUNDS; ++j) {
    const uint32_t quad = (uint32_t)j * TB + threadIdx.x;
    const uint64_t col0 = tile0 + 4ull * quad;
    if (col0 >= total) break;
    const uint32_t mine = l_quad[quad];
    uint32_t prev = quad ? (uint32_t)(l_quad[quad - 1] >> 3) & 1u : l_prev;
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t eq = mine >> i & 1u;
      if (col0 + i < total && ((mine >> (4 + i) & 1u) || eq != prev)) out |= (1u | eq << 1) << (8 * i);
      prev = eq;
    }
    *reinterpret_cast<uint32_t*>(flags + col0) = out;  // (flags: an arena block of a multiple of four bytes; col0: a multiple of four)
  }
}

struct Items {
  uint64_t n_items;
  uint32_t n_generated;
  const uint32_t* list;  // [n_generated] the boundary columns, ascending
  uint2* item;           // [n_items] x: the length (generated) or the first byte in the text (verbatim); y: letter (0: verbatim) | bytes << 8
  uint64_t* L;           // [n_items + 1] the byte lengths, then their inclusive sums behind L[0] = 0
};

__global__ __launch_bounds__(TB) void eqx_generated_kernel(CigarSet S, OpArrays A, Items I, const uint8_t* __restrict__ flags, uint64_t total) {
  const uint64_t g = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (g >= I.n_generated) return;
  const uint64_t col = I.list[g], next = g + 1 < I.n_generated ? I.list[g + 1] : total;
  const uint32_t r = op_at(A.C, 0, (uint32_t)(S.ops - 1), col);
  const uint64_t at = A.NC[r] + g;
  const uint32_t length = (uint32_t)(next - col), bytes = decimal_digits(length) + 1;
  I.item[at] = make_uint2(length, (flags[col] & 2 ? (uint32_t)'=' : (uint32_t)'X') | bytes << 8);
  I.L[at + 1] = bytes;
}

__global__ __launch_bounds__(TB) void eqx_verbatim_kernel(CigarSet S, OpArrays A, Items I) {
  const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (r >= S.ops) return;
  const uint32_t b = A.cls[r];
  if (!(b & B_VERBATIM)) return;
  const uint64_t at = A.NC[r] + rank_below(I.list, I.n_generated, A.C[r]);
  // the op's bytes: from behind the previous letter, or from the entry's first byte (the entry in front may end in digits)
  const uint64_t from = b & B_ENTRY_FIRST ? S.offset[entry_at(S.op_first, 0, (uint32_t)(S.k - 1), (uint32_t)r)] : (uint64_t)A.pos[r - 1] + 1;
  const uint32_t bytes = (uint32_t)(A.pos[r] + 1 - from);  // (at most 11: the entry has state 0)
  I.item[at] = make_uint2((uint32_t)from, bytes << 8);
  I.L[at + 1] = bytes;
}

__global__ __launch_bounds__(TB) void eqx_finish_kernel(CigarSet S, OpArrays A, Items I, const uint8_t* __restrict__ usable, swg_eqx_entry* __restrict__ entries,
                                                        unsigned long long* __restrict__ scalars) {
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  unsigned long long v[7] = {0, 0, 0, 0, 0, 0, 0};  // changed, then the six sums
  if (j < S.k && usable[j]) {
    const uint32_t first = S.op_first[j], end = S.op_first[j + 1];
    const uint64_t i0 = A.NC[first] + rank_below(I.list, I.n_generated, A.C[first]), i1 = A.NC[end] + rank_below(I.list, I.n_generated, A.C[end]);
    swg_eqx_entry e = entries[j];
    const uint64_t cols = S.P.A[end] - S.P.A[first];
    e.out_ops = (uint32_t)(i1 - i0);
    e.text_first = I.L[i0];
    e.text_len = (uint32_t)(I.L[i1] - I.L[i0]);
    e.inserted = (uint32_t)(S.P.X[end] - S.P.X[first] - cols);
    e.deleted = (uint32_t)(S.P.Y[end] - S.P.Y[first] - cols - e.deleted);  // (eqx_ops left the bases under N ops here)
    e.block = (uint64_t)e.matches + e.mismatches + e.inserted + e.deleted;
    // the bytes differ exactly when a column changes its letter, an op is split, merged or dropped, or a length loses leading zeros
    const bool changed = e.m_columns || e.eq_wrong || e.x_wrong || e.out_ops != end - first || e.text_len != S.offset[j + 1] - S.offset[j];
    e.flags = SWG_EQX_USABLE | (changed ? SWG_EQX_CHANGED : 0u);
    entries[j] = e;
    v[0] = changed, v[1] = e.matches, v[2] = e.mismatches, v[3] = e.n_columns, v[4] = e.eq_wrong, v[5] = e.x_wrong, v[6] = e.m_columns;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const unsigned long long s = wave_sum(v[i]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&scalars[F_CHANGED + i], s);
  }
}

// the last item i in [0, n) with L[i] <= o: the item that holds output byte o (every item has two bytes or more)
__device__ __forceinline__ uint64_t item_at(const uint64_t* __restrict__ L, uint64_t n, uint64_t o) {
  uint64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo + 1) >> 1);
    if (L[mid] <= o) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(TB) void eqx_text_kernel(Items I, const char* __restrict__ text, uint64_t text_bytes, char* __restrict__ out) {
  __shared__ uint32_t l_text[TTILE / 4];
  __shared__ uint64_t l_span[2];
  uint8_t* const l_byte = reinterpret_cast<uint8_t*>(l_text);
  const uint64_t tile0 = (uint64_t)blockIdx.x * TTILE;
  const uint32_t len = text_bytes - tile0 < (uint64_t)TTILE ? (uint32_t)(text_bytes - tile0) : (uint32_t)TTILE;
  if (threadIdx.x == 0) l_span[0] = item_at(I.L, I.n_items, tile0);
  if (threadIdx.x == 64) l_span[1] = item_at(I.L, I.n_items, tile0 + len - 1);
  __syncthreads();
  const uint64_t last = l_span[1];
  for (uint64_t i = l_span[0] + threadIdx.x; i <= last; i += TB) {
    const uint2 it = I.item[i];
    const uint64_t at = I.L[i];
    const uint32_t bytes = it.y >> 8, letter = it.y & 255u;
    for (uint32_t k = 0; k < bytes; ++k) {
      const uint64_t o = at + k;
      if (o < tile0 || o >= tile0 + len) continue;  // (an item across the tile's border: the neighbour writes the rest)
      l_byte[o - tile0] = letter ? op_text_byte(it.x, (uint8_t)letter, k) : (uint8_t)text[it.x + k];
    }
  }
  __syncthreads();
  for (uint32_t w = threadIdx.x; w * 4 < len; w += TB) {
    if (w * 4 + 4 <= len) {
      reinterpret_cast<uint32_t*>(out + tile0)[w] = l_text[w];  // (out: an arena block, 16-byte aligned; tile0: a multiple of four)
    } else {
      for (uint32_t b = w * 4; b < len; ++b) out[tile0 + b] = (char)l_byte[b];
    }
  }
}

// where: 0 = everything on the host, 1 = everything on the device, 2 = the host's, but seqs->bases in device memory
int eqx_run(swg_ctx* ctx, const swg_records* rec, int where, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
            swg_eqx_request* req) {
  const bool on_device = where == 1;
  static const char* const who = "eqx_records";
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL records or request", who);
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: reserved must be 0", who);
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
  req->ops = req->cigar_bad = req->empty = req->usable = req->no_sequence = req->out_of_sequence = req->columns = req->out_ops = req->text_bytes = req->changed = 0;
  req->matches = req->mismatches = req->n_columns = req->eq_wrong = req->x_wrong = req->m_columns = 0;
  if (!k) return SWG_OK;  // no device work
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)(on_device ? 0 : n * 26 + (size_t)n_seq * 8 + (where == 0 ? n_bases : 0)) + (size_t)B * 32 + (size_t)k * 80 + (size_t(4) << 20)));
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
        SWG_LAUNCH(ctx, "eqx_offsets", eqx_offsets_kernel<<<grid_of(n_seq), TB, 0, st>>>(Q.offset, n_seq, scalars));
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
    uint8_t* kind = swg_alloc<uint8_t>(ctx, ops + 1);
    uint32_t* pos = swg_alloc<uint32_t>(ctx, ops + 1);
    A.cls = swg_alloc<uint8_t>(ctx, ops + 1);
    A.C = swg_alloc<uint64_t>(ctx, ops + 1);
    A.NC = swg_alloc<uint64_t>(ctx, ops + 1);
    uint8_t* usable = swg_alloc<uint8_t>(ctx, k);
    swg_eqx_entry* entries = swg_alloc<swg_eqx_entry>(ctx, k);
    SWG_CHECK_ARENA(ctx);
    A.kind = kind, A.pos = pos;
    if (S.B) {
      const int aligned = (reinterpret_cast<uintptr_t>(S.text) & 15) == 0;
      SWG_LAUNCH(ctx, "eqx_letters", eqx_letters_kernel<<<grid_of((S.B + 15) / 16), TB, 0, st>>>(S, aligned, kind, pos));
      SWG_KERNEL_CHECK(ctx);
    }
    SWG_LAUNCH(ctx, "eqx_entries", eqx_entries_kernel<<<grid_of(k), TB, 0, st>>>(S, c, n_seq, req->set, Q.offset, usable, entries, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_HIP(ctx, hipMemsetAsync(A.C, 0, sizeof(uint64_t), st));
    SWG_HIP(ctx, hipMemsetAsync(A.NC, 0, sizeof(uint64_t), st));
    uint64_t total = 0, n_verbatim = 0;
    if (ops) {
      SWG_LAUNCH(ctx, "eqx_ops", eqx_ops_kernel<<<grid_of(ops), TB, 0, st>>>(S, A, usable, entries));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, A.C, A.C, ops + 1));
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, A.NC, A.NC, ops + 1));
      SWG_TRY(swg_read_scalars(ctx, A.C + ops, &total, 1));
      SWG_TRY(swg_read_scalars(ctx, A.NC + ops, &n_verbatim, 1));
    }
    uint64_t h[F_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, d_scalars, h, F_TOTAL));
    if (h[F_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: a record of the set has a sequence id >= n_seq", who);
    if (total >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 columns or more in one call", who);
    Items I{};
    uint8_t* flags = nullptr;
    if (total) {
      flags = swg_alloc<uint8_t>(ctx, (total + 3) & ~uint64_t(3));
      SWG_CHECK_ARENA(ctx);
      SWG_LAUNCH_N(ctx, "eqx_columns", total, eqx_columns_kernel<<<(unsigned)((total + CTILE - 1) / CTILE), TB, 0, st>>>(S, c, Q, A, total, entries, flags));
      SWG_KERNEL_CHECK(ctx);
      swg_flag_scan fs{};
      uint64_t n_generated = 0;
      SWG_TRY(swg_flags_count(ctx, flags, total, &fs, d_scalars + F_GENERATED));
      SWG_TRY(swg_read_scalars(ctx, d_scalars + F_GENERATED, &n_generated, 1));
      I.n_generated = (uint32_t)n_generated;  // (at most the columns)
      uint32_t* list = swg_alloc<uint32_t>(ctx, n_generated);
      SWG_CHECK_ARENA(ctx);
      SWG_TRY(swg_flags_compact(ctx, fs, list));
      I.list = list;
    }
    I.n_items = n_verbatim + I.n_generated;
    if (I.n_items >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 output ops or more in one call", who);
    I.item = swg_alloc<uint2>(ctx, I.n_items);
    I.L = swg_alloc<uint64_t>(ctx, I.n_items + 1);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(I.L, 0, sizeof(uint64_t), st));
    uint64_t text_bytes = 0;
    if (I.n_items) {
      if (I.n_generated) {
        SWG_LAUNCH_N(ctx, "eqx_generated", I.n_generated, eqx_generated_kernel<<<grid_of(I.n_generated), TB, 0, st>>>(S, A, I, flags, total));
        SWG_KERNEL_CHECK(ctx);
      }
      if (n_verbatim) {
        SWG_LAUNCH_N(ctx, "eqx_verbatim", ops, eqx_verbatim_kernel<<<grid_of(ops), TB, 0, st>>>(S, A, I));
        SWG_KERNEL_CHECK(ctx);
      }
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, I.L, I.L, I.n_items + 1));
      SWG_TRY(swg_read_scalars(ctx, I.L + I.n_items, &text_bytes, 1));
      if (text_bytes >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of output text or more in one call", who);
    }
    SWG_LAUNCH(ctx, "eqx_finish", eqx_finish_kernel<<<grid_of(k), TB, 0, st>>>(S, A, I, usable, entries, scalars));
    SWG_KERNEL_CHECK(ctx);
    if (req->text && text_bytes && text_bytes <= req->text_capacity) {
      char* out = swg_alloc<char>(ctx, text_bytes);
      SWG_CHECK_ARENA(ctx);
      SWG_LAUNCH_N(ctx, "eqx_text", text_bytes, eqx_text_kernel<<<(unsigned)((text_bytes + TTILE - 1) / TTILE), TB, 0, st>>>(I, S.text, text_bytes, out));
      SWG_KERNEL_CHECK(ctx);
      SWG_HIP(ctx, hipMemcpyAsync(req->text, out, text_bytes, hipMemcpyDeviceToHost, st));
    }
    if (req->entries && k <= req->entry_capacity) SWG_HIP(ctx, hipMemcpyAsync(req->entries, entries, k * sizeof(swg_eqx_entry), hipMemcpyDeviceToHost, st));
    uint64_t f[F_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, d_scalars, f, F_TOTAL));  // (synchronises: the copies above are done)
    req->ops = ops, req->cigar_bad = f[C_BAD_ENTRIES], req->empty = f[F_EMPTY], req->usable = f[F_USABLE];
    req->no_sequence = f[F_NO_SEQ], req->out_of_sequence = f[F_OUT_SEQ];
    req->columns = total, req->out_ops = I.n_items, req->text_bytes = text_bytes, req->changed = f[F_CHANGED];
    req->matches = f[F_SUMS], req->mismatches = f[F_SUMS + 1], req->n_columns = f[F_SUMS + 2];
    req->eq_wrong = f[F_SUMS + 3], req->x_wrong = f[F_SUMS + 4], req->m_columns = f[F_SUMS + 5];
    return SWG_OK;
  });
}

}  // namespace

int swg_eqx_run(swg_ctx* ctx, const swg_records* rec, int where, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                swg_eqx_request* req) {
  try {
    return eqx_run(ctx, rec, where, status, cigars, seqs, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_eqx_records(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                               swg_eqx_request* req) {
  return swg_eqx_run(ctx, rec, 0, status, cigars, seqs, req);
}
extern "C" int swg_eqx_records_device(swg_ctx* ctx, const swg_records* rec, const uint8_t* status, const swg_cigar_set* cigars, const swg_seq_set* seqs,
                                      swg_eqx_request* req) {
  return swg_eqx_run(ctx, rec, 1, status, cigars, seqs, req);
}
