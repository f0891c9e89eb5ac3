// The integer rules of the base-exact lift as plain functions: one op read back from its letter, what an op
// advances, and a row refined from the prefix sums of its record by binary searches.  swg_cigar.hip calls them from its kernels; a
// host compiler takes the file as it is, so the same text can be run on a CPU against the brute-force model.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SWG_CIGAR_FN __host__ __device__ __forceinline__
#else
#define SWG_CIGAR_FN inline
#endif

namespace swg_cigar {

// entry states (include/sweepga_gpu.h)
enum : uint32_t { ST_SYNTAX = 1, ST_VALUE = 2, ST_QSUM = 4, ST_TSUM = 8, ST_EMPTY = 16 };

SWG_CIGAR_FN bool is_digit(unsigned char ch) { return (unsigned)(ch - '0') < 10u; }

// what the op `ch` of length l adds to the four sums: query advance, target advance, aligned columns, '=' columns.  A byte that is
// no op letter adds nothing and is a syntax error.
SWG_CIGAR_FN uint32_t op_advance(unsigned char ch, uint64_t l, uint64_t* dx, uint64_t* dy, uint64_t* da, uint64_t* de) {
  *dx = *dy = *da = *de = 0;
  switch (ch) {
    case '=': *de = l; [[fallthrough]];
    case 'M':
    case 'X': *dx = *dy = *da = l; return 0;
    case 'I': *dx = l; return 0;
    case 'D':
    case 'N': *dy = l; return 0;
    case 'S':
    case 'H':
    case 'P': return 0;
    default: return ST_SYNTAX;
  }
}

// The number in front of the non-digit byte at `pos`, read backwards down to the previous non-digit byte or to `first`, the entry's
// first byte: 1 to 10 digits and a value below 2^32, or an error (the value is then 0).  At most 11 bytes are read, all of them
// inside [first, pos).
SWG_CIGAR_FN uint32_t op_number(const char* text, uint64_t first, uint64_t pos, uint32_t* value) {
  uint64_t v = 0, scale = 1;
  int digits = 0;
  *value = 0;
  for (uint64_t q = pos; q > first && digits <= 10; --q) {
    const unsigned char ch = (unsigned char)text[q - 1];
    if (!is_digit(ch)) break;
    if (digits < 10) v += (uint64_t)(ch - '0') * scale, scale *= 10;
    ++digits;
  }
  if (digits == 0 || digits > 10) return ST_SYNTAX;
  if (v >> 32) return ST_VALUE;
  *value = (uint32_t)v;
  return 0;
}

// The exclusive prefix sums of one call, ops + 1 entries each, over all entries' ops laid end to end: query advance, target
// advance, aligned columns, '=' columns.  A record's sums are differences against the value at its first op.
struct Prefix {
  const uint64_t *X, *Y, *A, *E;
};

// the last i in [0, cnt] with a[i] - a[0] <= v (a holds cnt + 1 non-decreasing values)
SWG_CIGAR_FN uint32_t last_le(const uint64_t* a, uint32_t cnt, uint64_t v) {
  const uint64_t base = a[0];
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (a[mid] - base <= v) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the aligned columns (*g) and the '=' columns (*h) whose offset along S lies below u; an op that u cuts counts with its part below u
SWG_CIGAR_FN void columns_below(const uint64_t* S, const uint64_t* A, const uint64_t* E, uint32_t nops, uint64_t u, uint64_t* g, uint64_t* h) {
  const uint32_t i = last_le(S, nops, u);
  *g = A[i] - A[0];
  *h = E[i] - E[0];
  if (i == nops) return;
  const uint64_t part = u - (S[i] - S[0]);  // op i advances S and holds offset u
  if (A[i + 1] > A[i]) *g += part;
  if (E[i + 1] > E[i]) *h += part;
}

// the offset along W of aligned column number g (g below the record's aligned total)
SWG_CIGAR_FN uint64_t column_offset(const uint64_t* A, const uint64_t* W, uint32_t nops, uint64_t g) {
  const uint32_t i = last_le(A, nops, g);
  return W[i] - W[0] + (g - (A[i] - A[0]));
}

// One exact row.  first, nops: the record's ops in P; axis 0: the query side is the source; [ca, cb) the clip on the source side.
SWG_CIGAR_FN void refine(const Prefix& P, uint64_t first, uint32_t nops, uint32_t axis, uint32_t minus, uint32_t ca, uint32_t cb, uint32_t q_start,
                         uint32_t q_end, uint32_t t_start, uint32_t t_end, uint32_t* dst_start, uint32_t* dst_end, uint32_t* aligned, uint32_t* matches) {
  const uint64_t* S = (axis ? P.Y : P.X) + first;  // the walk's offsets along the source and along the destination
  const uint64_t* W = (axis ? P.X : P.Y) + first;
  const uint64_t *A = P.A + first, *E = P.E + first;
  uint64_t u0, u1;  // the clip as offsets of the walk: a '-' record walks its query from q_end - 1 downwards
  if (axis) u0 = ca - t_start, u1 = cb - t_start;
  else if (minus) u0 = q_end - cb, u1 = q_end - ca;
  else u0 = ca - q_start, u1 = cb - q_start;
  uint64_t g0, h0, g1, h1;
  columns_below(S, A, E, nops, u0, &g0, &h0);
  columns_below(S, A, E, nops, u1, &g1, &h1);
  *aligned = (uint32_t)(g1 - g0);
  *matches = (uint32_t)(h1 - h0);
  if (g1 > g0) {
    const uint64_t w0 = column_offset(A, W, nops, g0), w1 = column_offset(A, W, nops, g1 - 1);
    if (!axis) *dst_start = t_start + (uint32_t)w0, *dst_end = t_start + (uint32_t)w1 + 1;
    else if (minus) *dst_start = q_end - 1 - (uint32_t)w1, *dst_end = q_end - (uint32_t)w0;
    else *dst_start = q_start + (uint32_t)w0, *dst_end = q_start + (uint32_t)w1 + 1;
    return;
  }
  uint32_t p;  // no column in the clip: the point behind the columns below ca
  if (!axis && minus) {  // below ca on the query = later in the walk: the first column behind the clip
    p = g1 < A[nops] - A[0] ? t_start + (uint32_t)column_offset(A, W, nops, g1) : t_end;
  } else {               // below ca = earlier in the walk: the last column in front of the clip
    const bool have = g0 > 0;
    const uint32_t w = have ? (uint32_t)column_offset(A, W, nops, g0 - 1) : 0u;
    if (!axis) p = have ? t_start + w + 1 : t_start;
    else if (minus) p = have ? q_end - 1 - w : q_end;
    else p = have ? q_start + w + 1 : q_start;
  }
  *dst_start = *dst_end = p;
}

}  // namespace swg_cigar
