// The integer rules of the chain files as plain functions: the marks that find the block starts, one block
// and one chain from the prefix sums, and a block's line.  swg_ucsc.hip calls them from its kernels; a host compiler takes the file
// as it is.
#pragma once
#include <stdint.h>

#include "swg_cigar_walk.h"

namespace swg_ucsc {

using swg_cigar::Prefix;
constexpr uint32_t ST_BEYOND = 32;
// what ucsc_entries leaves in the flag byte of an entry's first op
constexpr uint8_t BORDER = 2, BORDER_DEAD = 3;

// Two marks per op position r, both growing with r, so that a running maximum is "the last one":
//   the advancing mark of an op that adds to x or y: (r + 1) << 1 | aligned
//   the border mark of an entry's first op:          (r + 1) << 1 | dead   (dead: the entry gives no chain)
SWG_CIGAR_FN uint64_t mark_of(uint64_t r, uint32_t low) { return ((r + 1) << 1) | low; }
SWG_CIGAR_FN bool op_advances(const Prefix& P, uint64_t r) { return P.X[r + 1] != P.X[r] || P.Y[r + 1] != P.Y[r]; }
SWG_CIGAR_FN bool op_aligned(const Prefix& P, uint64_t r) { return P.A[r + 1] != P.A[r]; }
// An aligned op is a block start when the last advancing op in front of it is not aligned or lies in front of its entry's border.
// adv: the last advancing mark in front of the op (0: none); border: the last border mark at or in front of the op (never 0).
SWG_CIGAR_FN bool is_block_start(bool aligned, uint64_t adv, uint64_t border) {
  if (!aligned || (border & 1u)) return false;
  return (adv >> 1) < (border >> 1) || !(adv & 1u);  // (adv's position + 1 below the border's: in an earlier entry)
}

// Output block p of a chain of B blocks whose starts are s[0 .. B) (op positions) and whose entry ends at op e.
// reversed: the '-' strand seen from the query; swapped: from = query.
SWG_CIGAR_FN void block_of(const Prefix& P, const uint32_t* s, uint32_t B, uint32_t e, uint32_t p, bool reversed, bool swapped, uint32_t* size,
                           uint32_t* dt, uint32_t* dq) {
  const uint32_t js = reversed ? B - 1 - p : p;
  const uint64_t a0 = P.A[s[js]], a1 = P.A[js + 1 < B ? s[js + 1] : e];
  *size = (uint32_t)(a1 - a0);
  *dt = *dq = 0;
  if (p + 1 >= B) return;
  const uint32_t g = reversed ? B - 2 - p : p;  // the gap behind block g
  const uint32_t u = s[g], v = s[g + 1];
  const uint64_t sz = P.A[v] - P.A[u];
  const uint32_t gq = (uint32_t)(P.X[v] - P.X[u] - sz), gt = (uint32_t)(P.Y[v] - P.Y[u] - sz);
  *dt = swapped ? gq : gt;
  *dq = swapped ? gt : gq;
}

// The four coordinates of a chain: x0, x1, y0, y1 its ends as walk offsets, Lq_seq / Lt_seq the sequences' lengths.
SWG_CIGAR_FN void chain_ends(bool minus, bool swapped, uint32_t q_start, uint32_t q_end, uint32_t t_start, uint32_t Lq_seq, uint32_t Lt_seq, uint64_t x0,
                             uint64_t x1, uint64_t y0, uint64_t y1, uint32_t* ref_start, uint32_t* ref_end, uint32_t* oth_start, uint32_t* oth_end) {
  const uint32_t ts = t_start + (uint32_t)y0, te = t_start + (uint32_t)y1;
  if (!swapped) {
    const uint32_t base = minus ? Lq_seq - q_end : q_start;
    *ref_start = ts, *ref_end = te, *oth_start = base + (uint32_t)x0, *oth_end = base + (uint32_t)x1;
  } else if (!minus) {
    *ref_start = q_start + (uint32_t)x0, *ref_end = q_start + (uint32_t)x1, *oth_start = ts, *oth_end = te;
  } else {
    *ref_start = q_end - (uint32_t)x1, *ref_end = q_end - (uint32_t)x0, *oth_start = Lt_seq - te, *oth_end = Lt_seq - ts;
  }
}

SWG_CIGAR_FN uint32_t digits10(uint32_t v) {
  return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u
       : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
// `size\tdt\tdq\n`, or `size\n\n` for a chain's last block: at most 33 bytes
SWG_CIGAR_FN uint32_t line_length(uint32_t size, uint32_t dt, uint32_t dq, bool last) {
  return last ? digits10(size) + 2u : digits10(size) + digits10(dt) + digits10(dq) + 3u;
}
SWG_CIGAR_FN uint32_t put_number(char* o, uint32_t v) {
  const uint32_t d = digits10(v);
  for (uint32_t k = d; k > 0; --k) o[k - 1] = (char)('0' + v % 10u), v /= 10u;
  return d;
}
SWG_CIGAR_FN uint32_t line_text(char* o, uint32_t size, uint32_t dt, uint32_t dq, bool last) {
  uint32_t n = put_number(o, size);
  if (last) {
    o[n++] = '\n', o[n++] = '\n';
    return n;
  }
  o[n++] = '\t';
  n += put_number(o + n, dt);
  o[n++] = '\t';
  n += put_number(o + n, dq);
  o[n++] = '\n';
  return n;
}

}  // namespace swg_ucsc
