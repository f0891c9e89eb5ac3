// The rules of the variant calls as plain functions: a base normalised and complemented, the counter of a
// compared column, and one variant -- its six words, its allele lengths and every allele byte -- from the site of its op.
// swg_variants.hip calls them from its kernels; a host compiler takes the file as it is.
#pragma once
#include <stdint.h>

#include "swg_diffs_walk.h"

namespace swg_variants {

using swg_diffs::K_DEL;
using swg_diffs::K_INS;
using swg_diffs::K_M;
using swg_diffs::K_SNP;

// A, C, G, T as 0 .. 3 in either case, every other byte 4 (N)
SWG_CIGAR_FN uint32_t code_of(uint8_t b) {
  switch (b | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
    default: return 4;
  }
}
SWG_CIGAR_FN uint32_t comp_code(uint32_t c) { return c < 4 ? 3u - c : 4u; }
SWG_CIGAR_FN uint8_t letter_of(uint32_t c) { return (uint8_t)(0x4e54474341ull >> (8 * c)); }  // "ACGTN"

// the counters of a compared column, in the order of swg_variant_pair from sub[] on: 12 substitutions (REF-major, the diagonal left
// out), same, m_equal, n_columns
enum { C_SAME = 12, C_M_EQUAL = 13, C_N = 14, C_TOTAL = 15 };
SWG_CIGAR_FN int column_counter(uint32_t r, uint32_t a, bool under_m) {
  if (r == 4 || a == 4) return C_N;
  if (r == a) return under_m ? C_M_EQUAL : C_SAME;
  return (int)(r * 3 + a - (a > r ? 1u : 0u));
}

// Where an op lies: the record's sides and strand, the op's kind, length, walk offsets and p = t_start + y.  For an SNV x, p are
// the column's and l is 1.
struct Site {
  uint32_t kind, minus, l;
  uint32_t x;
  uint64_t p;
  uint32_t q_start, q_end;
};

// the index into the query sequence of the column at walk offset w
SWG_CIGAR_FN uint64_t query_index(const Site& s, uint64_t w) { return s.minus ? (uint64_t)s.q_end - 1 - w : (uint64_t)s.q_start + w; }
// the query column at walk offset w as a code; Q: the query sequence's first byte
SWG_CIGAR_FN uint32_t query_column(const Site& s, const uint8_t* Q, uint64_t w) {
  const uint32_t c = code_of(Q[query_index(s, w)]);
  return s.minus ? comp_code(c) : c;
}

// an indel's fate: 0 = a variant, 1 = unanchored, 2 = long
SWG_CIGAR_FN int indel_fate(uint32_t kind, uint64_t l, uint64_t p, uint64_t t_len, uint32_t max_indel) {
  if (kind == K_DEL && p == 0 && l == t_len) return 1;
  return max_indel && l > max_indel ? 2 : 0;
}

// the allele bytes of the site's variant: REF and ALT together
SWG_CIGAR_FN uint64_t allele_bytes(const Site& s) { return s.kind == K_SNP ? 2 : (uint64_t)s.l + 2; }

// words 2 .. 5 of the variant: pos, ref_len, alt_len, q_pos
SWG_CIGAR_FN void variant_words(const Site& s, uint32_t w[4]) {
  if (s.kind == K_SNP) {
    w[0] = (uint32_t)s.p, w[1] = w[2] = 1, w[3] = (uint32_t)query_index(s, s.x);
    return;
  }
  const bool ins = s.kind == K_INS;
  w[0] = s.p ? (uint32_t)(s.p - 1) : 0u;
  w[1] = ins ? 1u : s.l + 1, w[2] = ins ? s.l + 1 : 1u;
  w[3] = s.minus ? s.q_end - s.x - (ins ? s.l : 0u) : s.q_start + s.x;
}

// allele byte k of the variant (k < allele_bytes); T, Q: the first bytes of the target and the query sequence
SWG_CIGAR_FN uint8_t allele_byte(const Site& s, const uint8_t* T, const uint8_t* Q, uint64_t k) {
  const uint64_t l = s.l;
  if (s.kind == K_SNP) return letter_of(k == 0 ? code_of(T[s.p]) : query_column(s, Q, s.x));
  if (s.kind == K_INS) {
    if (s.p > 0) return letter_of(k < 2 ? code_of(T[s.p - 1]) : query_column(s, Q, s.x + (k - 2)));
    return letter_of(k == 0 || k == l + 1 ? code_of(T[0]) : query_column(s, Q, s.x + (k - 1)));
  }
  if (s.p > 0) return letter_of(code_of(T[k <= l ? s.p - 1 + k : s.p - 1]));  // a deletion: REF l + 1 bases, ALT one
  return letter_of(code_of(T[k <= l ? k : l]));
}

}  // namespace swg_variants
