// The integer rules of the difference list as plain functions: an op's kind from its letter, its length from
// the prefix differences, the row filter, the spectrum bin and one 32-byte row.  swg_diffs.hip calls them from its kernels; a host
// compiler takes the file as it is.
#pragma once
#include <stdint.h>

#include "swg_cigar_walk.h"

namespace swg_diffs {

using swg_cigar::Prefix;

// the kind byte of an op: the four row kinds are the ABI's SWG_DIFF_* bits, K_M marks an M op (its columns are counted, it gives no
// row); every other byte -- '=', S, H, P, a foreign byte -- is 0
constexpr uint32_t K_SNP = 1, K_INS = 2, K_DEL = 4, K_SKIP = 8, K_M = 16, K_ROWS = 15;

SWG_CIGAR_FN uint32_t kind_of(unsigned char ch) {
  switch (ch) {
    case 'X': return K_SNP;
    case 'I': return K_INS;
    case 'D': return K_DEL;
    case 'N': return K_SKIP;
    case 'M': return K_M;
    default: return 0;
  }
}

// the length of op r of kind `kind` (not 0): X and M make columns, I advances the query, D and N the target
SWG_CIGAR_FN uint64_t op_length(const Prefix& P, uint64_t r, uint32_t kind) {
  const uint64_t* a = kind & (K_SNP | K_M) ? P.A : kind & K_INS ? P.X : P.Y;
  return a[r + 1] - a[r];
}

// whether the op gives a row: its kind is asked for, it has a length, and an indel is at least min_indel long
SWG_CIGAR_FN bool is_row(uint32_t kind, uint64_t l, uint32_t kinds, uint32_t min_indel) {
  if (!(kind & kinds & K_ROWS) || l == 0) return false;
  return kind == K_SNP || l >= min_indel;
}

// the first index of the spectrum: SNP, INS, DEL, SKIP; and the bin, the bit length of l (1 .. 32 for 0 < l < 2^32)
SWG_CIGAR_FN int kind_index(uint32_t kind) { return kind & K_SNP ? 0 : kind & K_INS ? 1 : kind & K_DEL ? 2 : 3; }
SWG_CIGAR_FN int length_bin(uint64_t l) {
  const int bits = l ? 64 - __builtin_clzll(l) : 0;
  return bits < 32 ? bits : 32;
}

// The row of op r (a row kind, length > 0) of the entry whose ops are [first, end): eight 32-bit words in the order of swg_diff_row.
SWG_CIGAR_FN void row_of(const Prefix& P, uint32_t first, uint32_t end, uint32_t r, uint32_t kind, uint32_t record, bool minus, uint32_t q_start,
                         uint32_t q_end, uint32_t t_start, uint32_t w[8]) {
  const uint32_t l = (uint32_t)op_length(P, r, kind);
  const uint32_t x = (uint32_t)(P.X[r] - P.X[first]), y = (uint32_t)(P.Y[r] - P.Y[first]);
  const uint32_t lt = kind == K_INS ? 0u : l, lq = kind & (K_SNP | K_INS) ? l : 0u;
  w[0] = record, w[1] = kind | (minus ? 256u : 0u);
  w[2] = t_start + y, w[3] = t_start + y + lt;
  w[4] = minus ? q_end - x - lq : q_start + x;
  w[5] = minus ? q_end - x : q_start + x + lq;
  w[6] = r > first ? (uint32_t)(P.E[r] - P.E[r - 1]) : 0u;
  w[7] = r + 1 < end ? (uint32_t)(P.E[r + 2] - P.E[r + 1]) : 0u;
}

}  // namespace swg_diffs
