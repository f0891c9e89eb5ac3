// The integer rules of the lift slices as plain functions: one slice from the prefix sums of its record and
// the letter positions of its ops, its copy plan, and one byte of its text addressed from the output side.  swg_slice.hip calls them
// from its kernels; a host compiler takes the file as it is.
#pragma once
#include <stdint.h>

#include "swg_cigar_walk.h"
#include "swg_ucsc_walk.h"

namespace swg_slice {

using swg_cigar::Prefix;
using swg_ucsc::digits10;

// Where the bytes of a slice's text come from: `head` in decimal and its letter, `mid` bytes of the call's CIGAR text from `src`
// on, then -- tail_digits != 0 -- `tail` in decimal and its letter.
struct Plan {
  uint64_t src;
  uint32_t mid, head, tail;
  uint8_t head_letter, tail_letter, head_digits, tail_digits;
};  // 24 bytes

struct Slice {
  uint32_t q_start, q_end, t_start, t_end;
  uint32_t aligned, matches, text_len;
  bool has_eq;
  uint64_t block;
};

// The slice of one exact row.  first, nops: the record's ops in P; pos: the letter positions of those ops, relative to the entry's
// first byte `entry` of `text`; axis 0: the query side is the source; [ca, cb) the clip on the source side.  Returns the aligned
// columns inside the clip; *s and *p are written only when there are any.
SWG_CIGAR_FN uint32_t slice_of(const Prefix& P, uint64_t first, uint32_t nops, const uint32_t* pos, const char* text, uint64_t entry, uint32_t axis,
                               uint32_t minus, uint32_t ca, uint32_t cb, uint32_t q_start, uint32_t q_end, uint32_t t_start, Slice* s, Plan* p) {
  const uint64_t *X = P.X + first, *Y = P.Y + first, *A = P.A + first, *E = P.E + first;
  const uint64_t* S = axis ? Y : X;
  uint64_t u0, u1;  // the clip as offsets of the walk (swg_cigar::refine)
  if (axis) u0 = ca - t_start, u1 = cb - t_start;
  else if (minus) u0 = q_end - cb, u1 = q_end - ca;
  else u0 = ca - q_start, u1 = cb - q_start;
  uint64_t g0, h0, g1, h1;
  swg_cigar::columns_below(S, A, E, nops, u0, &g0, &h0);
  swg_cigar::columns_below(S, A, E, nops, u1, &g1, &h1);
  if (g1 <= g0) return 0;
  const uint32_t i0 = swg_cigar::last_le(A, nops, g0), i1 = swg_cigar::last_le(A, nops, g1 - 1);  // the ops that hold g0 and g1 - 1
  const uint64_t a0 = A[i0] - A[0], a1 = A[i1] - A[0];
  const uint64_t x0 = X[i0] - X[0] + (g0 - a0), x1 = X[i1] - X[0] + (g1 - 1 - a1);
  const uint64_t y0 = Y[i0] - Y[0] + (g0 - a0), y1 = Y[i1] - Y[0] + (g1 - 1 - a1);
  s->aligned = (uint32_t)(g1 - g0), s->matches = (uint32_t)(h1 - h0);
  s->t_start = t_start + (uint32_t)y0, s->t_end = t_start + (uint32_t)y1 + 1;
  if (minus) s->q_start = q_end - 1 - (uint32_t)x1, s->q_end = q_end - (uint32_t)x0;
  else s->q_start = q_start + (uint32_t)x0, s->q_end = q_start + (uint32_t)x1 + 1;
  s->block = (x1 - x0 + 1) + (y1 - y0 + 1) - (g1 - g0);
  s->has_eq = E[nops] != E[0];
  p->head_letter = (uint8_t)text[entry + pos[i0]];
  if (i0 == i1) {
    p->head = (uint32_t)(g1 - g0);
    p->src = 0, p->mid = 0, p->tail = 0, p->tail_letter = 0, p->tail_digits = 0;
  } else {
    p->head = (uint32_t)(A[i0 + 1] - A[0] - g0);
    p->src = entry + pos[i0] + 1, p->mid = pos[i1 - 1] - pos[i0];
    p->tail = (uint32_t)(g1 - a1), p->tail_letter = (uint8_t)text[entry + pos[i1]];
    p->tail_digits = (uint8_t)digits10(p->tail);
  }
  p->head_digits = (uint8_t)digits10(p->head);
  s->text_len = p->head_digits + 1u + p->mid + (p->tail_digits ? p->tail_digits + 1u : 0u);
  return s->aligned;
}

// digit number d from the right (0 = the units) of v
SWG_CIGAR_FN uint8_t digit_of(uint32_t v, uint32_t d) {
  const uint32_t p10 = d == 0 ? 1u : d == 1 ? 10u : d == 2 ? 100u : d == 3 ? 1000u : d == 4 ? 10000u : d == 5 ? 100000u : d == 6 ? 1000000u
                     : d == 7 ? 10000000u : d == 8 ? 100000000u : 1000000000u;
  return (uint8_t)('0' + v / p10 % 10u);
}

// byte `rel` of the text of a slice with plan p (rel below its text_len)
SWG_CIGAR_FN uint8_t text_byte(const Plan& p, const char* text, uint32_t rel) {
  if (rel < p.head_digits) return digit_of(p.head, p.head_digits - 1u - rel);
  if (rel == p.head_digits) return p.head_letter;
  rel -= p.head_digits + 1u;
  if (rel < p.mid) return (uint8_t)text[p.src + rel];
  rel -= p.mid;
  if (rel < p.tail_digits) return digit_of(p.tail, p.tail_digits - 1u - rel);
  return p.tail_letter;
}

}  // namespace swg_slice
