// The rules of the alignment blocks as plain functions: what an op gives to the two rows, which ops are
// breakers, where a candidate ends, a block's fields from the prefix sums, the byte of one row at one alignment column, and
// comp_raw.  swg_maf.hip calls them from its kernels; a host compiler takes the file as it is.
#pragma once
#include <stdint.h>

#include "../../include/sweepga_gpu.h"
#include "swg_cigar_walk.h"

namespace swg_maf {

using swg_cigar::Prefix;

// comp_raw as the header states it; the device keeps a copy of its own (swg_maf.hip)
static const uint8_t COMP_RAW[256] = SWG_MAF_COMP_RAW;
inline uint8_t comp_raw(uint8_t b) { return COMP_RAW[b]; }

// What an op gives, from its advances alone (dx on the query, dy on the target): bit 0 = target bytes, bit 1 = query bytes.  Both:
// M, = or X; the query alone: I; the target alone: D or N; 0: S, H, P or a length of 0 -- no columns.
enum : uint32_t { ROW_T = 1, ROW_Q = 2 };
SWG_CIGAR_FN uint32_t op_rows(uint64_t dx, uint64_t dy) { return (dy ? ROW_T : 0u) | (dx ? ROW_Q : 0u); }
// its alignment columns (an op advances both sides alike or one side only)
SWG_CIGAR_FN uint64_t op_columns(uint64_t dx, uint64_t dy) { return dx > dy ? dx : dy; }
// an I, D or N op of g bases or more, g > 0
SWG_CIGAR_FN bool is_breaker(uint64_t dx, uint64_t dy, uint32_t g) { return g != 0 && (dx == 0) != (dy == 0) && op_columns(dx, dy) >= g; }
SWG_CIGAR_FN bool op_is_breaker(const Prefix& P, uint64_t r, uint32_t g) { return is_breaker(P.X[r + 1] - P.X[r], P.Y[r + 1] - P.Y[r], g); }

// Where the candidate that starts at op `start` ends: `next` is the next candidate's start in the same entry, or the entry's op
// end; the breakers between the two stand directly in front of `next`.  bk_*: the breakers in front of the two ops.
SWG_CIGAR_FN uint64_t candidate_end(uint64_t next, uint64_t bk_next, uint64_t bk_start) { return next - (bk_next - bk_start); }

// The fields of the candidate of ops [start, end) of the entry whose first op is `first`, in the order of swg_maf_block's words
// 2 .. 11: op_first, op_end, t_start, t_bases, q_start (forward strand), q_bases, aligned, columns, flags, walk_x.
SWG_CIGAR_FN void block_words(const Prefix& P, uint64_t first, uint64_t start, uint64_t end, bool minus, uint32_t q_start, uint32_t q_end,
                              uint32_t t_start, uint32_t w[10]) {
  const uint32_t x0 = (uint32_t)(P.X[start] - P.X[first]), y0 = (uint32_t)(P.Y[start] - P.Y[first]);
  const uint32_t q_bases = (uint32_t)(P.X[end] - P.X[start]), t_bases = (uint32_t)(P.Y[end] - P.Y[start]), aligned = (uint32_t)(P.A[end] - P.A[start]);
  w[0] = (uint32_t)(start - first), w[1] = (uint32_t)(end - first);
  w[2] = t_start + y0, w[3] = t_bases;
  w[4] = minus ? q_end - x0 - q_bases : q_start + x0, w[5] = q_bases;
  w[6] = aligned, w[7] = q_bases + t_bases - aligned;
  w[8] = minus ? SWG_MAF_MINUS : 0u, w[9] = x0;
}

// Where one op's bytes lie: the index into the bases of its first target byte and of its first query byte (on '-' the columns
// descend from it), and what it gives to the rows.
struct OpBytes {
  uint64_t t_at, q_at;
  uint32_t rows, minus;
};
// the byte of row `row` (0 = target, 1 = query) at column d of the op; comp: the comp_raw table
SWG_CIGAR_FN uint8_t row_byte(const OpBytes& o, const uint8_t* bases, const uint8_t* comp, uint32_t row, uint64_t d) {
  if (row == 0) return o.rows & ROW_T ? bases[o.t_at + d] : (uint8_t)'-';
  if (!(o.rows & ROW_Q)) return (uint8_t)'-';
  return o.minus ? comp[bases[o.q_at - d]] : bases[o.q_at + d];
}

}  // namespace swg_maf
