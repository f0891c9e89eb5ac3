// The integer rules of the divergence track as plain functions: where an op lies on the axis, which quantity
// its bases add to, and the window arithmetic of an interval.  swg_divergence.hip calls them from its kernels; a host compiler takes
// the file as it is.
#pragma once
#include <stdint.h>

#include "swg_diffs_walk.h"

namespace swg_divergence {

using swg_cigar::Prefix;
using swg_diffs::K_DEL;
using swg_diffs::K_INS;
using swg_diffs::K_M;
using swg_diffs::K_SKIP;
using swg_diffs::K_SNP;

// what the op pass adds per window, in the order of its part of the table
enum { Q_MISMATCHES = 0, Q_M_COLUMNS, Q_UNALIGNED, Q_INSERTED, Q_RUNS, Q_INDELS, Q_OPS };
constexpr int Q_EXTENT = 3;  // the first three are bases along the axis: an op can spread them over several windows

// the flags of an entry word: the entry is usable and its record takes part; the walk descends along the axis (axis 0, '-' strand)
constexpr uint32_t E_USABLE = 1, E_DESCENDS = 2;

// The entry's origin: with it the axis coordinate of walk offset w (x on axis 0, y on axis 1) of op r is origin + (uint32_t)S[r] on an
// ascending walk and origin - (uint32_t)S[r] on a descending one, S = X or Y.  All coordinates lie below 2^32, so the arithmetic
// modulo 2^32 is exact and the entry's first prefix value need not travel.
SWG_CIGAR_FN uint32_t entry_origin(const Prefix& P, uint32_t first, uint32_t axis, bool minus, uint32_t q_start, uint32_t q_end, uint32_t t_start) {
  if (axis) return t_start - (uint32_t)P.Y[first];
  return minus ? q_end + (uint32_t)P.X[first] : q_start - (uint32_t)P.X[first];
}

// whether the op consumes bases of the axis: X and M always, I on the query axis, D and N on the target axis
SWG_CIGAR_FN bool has_extent(uint32_t kind, uint32_t axis) {
  return (kind & (K_SNP | K_M)) != 0 || (axis ? (kind & (K_DEL | K_SKIP)) != 0 : (kind & K_INS) != 0);
}

// the quantity the bases of an op with extent add to
SWG_CIGAR_FN int extent_quantity(uint32_t kind) { return kind & K_SNP ? Q_MISMATCHES : kind & K_M ? Q_M_COLUMNS : Q_UNALIGNED; }

// Where op r (kind not 0, length l > 0) of an entry with `origin`, `flags` and axis end b lies: [*lo, *hi) for an op with extent; for
// one without (its l bases are the other sequence's) the one base min(p, b - 1) whose window takes it.
SWG_CIGAR_FN void op_where(const Prefix& P, uint64_t r, uint32_t axis, uint32_t flags, uint32_t origin, uint32_t b, bool extent, uint32_t l, uint32_t* lo,
                           uint32_t* hi) {
  const uint32_t w = (uint32_t)(axis ? P.Y[r] : P.X[r]), on_axis = extent ? l : 0u;
  if (flags & E_DESCENDS) *hi = origin - w, *lo = *hi - on_axis;
  else *lo = origin + w, *hi = *lo + on_axis;
  if (!extent) {
    const uint32_t p = *lo;  // a <= p <= b
    *lo = p < b ? p : b - 1;
    *hi = *lo + 1;
  }
}

// [lo, hi), lo < hi, over windows of W bases: the first and the last window, and what the interval has in each (for k0 == k1 all of
// it is in *in0 and *in1 is 0); the windows between the two are filled
SWG_CIGAR_FN void window_span(uint32_t lo, uint32_t hi, uint32_t W, uint32_t* k0, uint32_t* k1, uint64_t* in0, uint64_t* in1) {
  *k0 = lo / W, *k1 = (hi - 1) / W;
  if (*k0 == *k1) {
    *in0 = hi - lo, *in1 = 0;
  } else {
    *in0 = (*k0 + 1ull) * W - lo;
    *in1 = hi - (uint64_t)*k1 * W;
  }
}

}  // namespace swg_divergence
