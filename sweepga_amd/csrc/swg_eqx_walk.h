// The rules of the resolved CIGARs as plain functions: whether a column is equal, what kind of op a letter
// is and where a column run starts, the decimal digits of a length and byte k of `<length><letter>`, and the six sums of a column.
// swg_eqx.hip calls them from its kernels; a host compiler takes the file as it is.
#pragma once
#include <stdint.h>

#include "swg_variants_walk.h"

namespace swg_eqx {

using swg_variants::code_of;
using swg_variants::comp_code;

// the class of an op by its letter: the three column ops, 0 for every other byte
enum : uint32_t { L_M = 1, L_EQ = 2, L_X = 3 };
SWG_CIGAR_FN uint32_t column_class(unsigned char ch) { return ch == 'M' ? L_M : ch == '=' ? L_EQ : ch == 'X' ? L_X : 0u; }
SWG_CIGAR_FN bool is_column_op(unsigned char ch) { return column_class(ch) != 0; }
// an op starts a column run when it is a column op and the op in front of it (prev: its letter, 0 = the entry's first op) is none
SWG_CIGAR_FN bool is_run_start(unsigned char ch, unsigned char prev) { return is_column_op(ch) && !is_column_op(prev); }

// r: the target's code, a: the query column's code (swg_variants_walk.h: 0 .. 3 a base, 4 = N).  A column with an N is never equal.
SWG_CIGAR_FN bool column_eq(uint32_t r, uint32_t a) { return r == a && r != 4; }
SWG_CIGAR_FN bool column_n(uint32_t r, uint32_t a) { return r == 4 || a == 4; }

// the decimal digits of a length: 1 .. 10
SWG_CIGAR_FN uint32_t decimal_digits(uint32_t v) {
  uint32_t d = 1;
  for (uint32_t p = 10; d < 10 && v >= p; p *= 10) ++d;
  return d;
}
// byte k of `<length><letter>`, k <= decimal_digits(length)
SWG_CIGAR_FN uint8_t op_text_byte(uint32_t length, uint8_t letter, uint32_t k) {
  const uint32_t d = decimal_digits(length);
  if (k >= d) return letter;
  uint32_t v = length;
  for (uint32_t i = d - 1; i > k; --i) v /= 10;
  return (uint8_t)('0' + v % 10);
}

// The six sums of one entry, 21 bits each in two words, so that a lane adds the columns of a tile (at most 2^12) and a wavefront
// folds its lanes (2^18) without a carry between the fields: [0] matches, mismatches, n_columns; [1] eq_wrong, x_wrong, m_columns.
enum { SUM_BITS = 21 };
struct ColumnSums {
  unsigned long long w[2];
};
SWG_CIGAR_FN void sums_add(ColumnSums& s, uint32_t cls, bool eq, bool n) {
  s.w[0] += (eq ? 1ull : 1ull << SUM_BITS) + (n ? 1ull << (2 * SUM_BITS) : 0ull);
  s.w[1] += (cls == L_EQ && !eq ? 1ull : 0ull) + (cls == L_X && eq ? 1ull << SUM_BITS : 0ull) + (cls == L_M ? 1ull << (2 * SUM_BITS) : 0ull);
}
SWG_CIGAR_FN uint32_t sums_field(const ColumnSums& s, int i) { return (uint32_t)(s.w[i / 3] >> (SUM_BITS * (i % 3))) & ((1u << SUM_BITS) - 1u); }

}  // namespace swg_eqx
